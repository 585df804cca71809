// run.cpp — the streaming engine: one sid run, pileup text in, CSV out, over
// line-aligned chunks with bounded host memory (include/sid.h "streaming
// engine").
//
// It replaces the reference's whole-input flow -- readFile materialising
// every site (call.cpp:11-20), callX over the vector (call.cpp:62-289), the
// output loop (sid.cpp:102-105) -- by a pipeline per device:
//
//   uploader   source chunk -> device text buffer (ring of `slots`, or a
//              retained buffer); H2D on its own stream
//   compute    line index -> (sync: sites) -> parse -> call -> record lengths
//              -> (sync: bytes) -> records into a device CSV buffer
//   drain      CSV buffer -> pinned ring -> writer (D2H on its own stream)
//   writer     one for all devices: write() in chunk = file order
//
// Two passes keep the reference's all-or-nothing output (a malformed line
// aborts before anything is printed):
//   pass 1  every chunk is indexed and parsed (validation); -m local / quality
//           also call and format it, the records held in HBM (hold budget);
//           the Lynch methods accumulate the profile histogram instead.
//   (first error in file order -> return it, nothing written)
//   (Lynch: merge the device histograms, one estimate, class tables)
//   pass 2  header, then every chunk in file order: held records are copied
//           back as they are; the others are processed again from their text
//           (kept in HBM within the retain budget, else read again).
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <pthread.h>
#include <sched.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "bgzf_dev.h"
#include "context.h"
#include "windows.h"
#include "depth_hist.h"
#include "region_stats.h"
#include "sid_internal.h"
#include "strip.h"
#include "synth.h"

namespace {

constexpr uint64_t PAD = 256;   // readable bytes past every chunk's end (16-B windows, zeroed)

double wall()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// bounded blocking queue; close() wakes every waiter (push fails, pop drains)
template <class T>
class Chan {
public:
    bool push(T v)
    {
        std::unique_lock<std::mutex> l(m_);
        if (closed_) return false;
        q_.push_back(std::move(v));
        cv_.notify_one();
        return true;
    }
    bool pop(T& v)
    {
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [&] { return !q_.empty() || closed_; });
        if (q_.empty()) return false;
        v = std::move(q_.front());
        q_.pop_front();
        return true;
    }
    // without waiting: false when nothing is queued right now
    bool try_pop(T& v)
    {
        std::lock_guard<std::mutex> l(m_);
        if (q_.empty()) return false;
        v = std::move(q_.front());
        q_.pop_front();
        return true;
    }
    void close()
    {
        std::lock_guard<std::mutex> l(m_);
        closed_ = true;
        cv_.notify_all();
    }
    void reset()
    {
        std::lock_guard<std::mutex> l(m_);
        q_.clear();
        closed_ = false;
    }

private:
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<T> q_;
    bool closed_ = false;
};

// Device buffers reused across chunks and runs (hipMalloc/hipFree are slow and
// hipFree waits for the device).  A buffer returned with an event is reused
// on another stream only after that event.
class DevPool {
public:
    int device = 0;
    ~DevPool() { release(); }
    // A fitting buffer whose last use is done is taken first; while every
    // fitting one is still in use (its event pending), up to two of them, a
    // new one is allocated rather than waited for -- the records' buffer of
    // a chunk is in use until its D2H completes, and the next chunk's writer
    // waiting for that copy serialised writer and D2H chunk after chunk (the
    // PCIe leg's last chunks then drained one D2H at a time after the last
    // upload)
    char* get(uint64_t need, uint64_t* cap, hipStream_t st)
    {
        std::lock_guard<std::mutex> l(m_);
        const uint64_t top = 2 * need + (64u << 20);
        const auto lo = free_.lower_bound(need);
        auto it = free_.end();
        int busy = 0;
        for (auto jt = lo; jt != free_.end() && jt->first <= top; ++jt) {
            if (!jt->second.ev || jt->second.st == st) {   // (returned on this stream: ordered, no wait)
                it = jt;
                break;
            }
            const hipError_t q = hipEventQuery(jt->second.ev);
            if (q == hipSuccess) {
                it = jt;
                break;
            }
            (void)hipGetLastError();   // (hipErrorNotReady: not an error of this thread's work)
            ++busy;
        }
        if (it == free_.end() && busy >= 2) it = lo;   // (growth bounded: wait for the first)
        if (it != free_.end()) {
            Entry en = it->second;
            *cap = it->first;
            free_.erase(it);
            if (en.ev) {
                (void)hipStreamWaitEvent(st, en.ev, 0);
                evs_.push_back(en.ev);
            }
            return en.p;
        }
        const uint64_t c = (need + PAD + (4u << 20) - 1) & ~(uint64_t)((4u << 20) - 1);
        char* p = nullptr;
        if (hipMalloc(&p, c) != hipSuccess) {
            // the caller falls back (ring slot, pass 2, arena): clear the
            // runtime's sticky last error, or the next launch check on this
            // thread (hipGetLastError) reports this failed allocation
            (void)hipGetLastError();
            return nullptr;
        }
        all_.push_back(p);
        bytes_ += c;
        *cap = c;
        return p;
    }
    // `after` (may be null): the buffer is free once the work before it on
    // its stream has run
    void put(char* p, uint64_t cap, hipStream_t after)
    {
        if (!p || !cap) return;   // cap 0: not a pooled buffer (the hold arena)
        std::lock_guard<std::mutex> l(m_);
        Entry en{p, nullptr, after};
        if (after) {
            if (evs_.empty()) {
                hipEvent_t ev;
                if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess) evs_.push_back(ev);
            }
            if (!evs_.empty()) {
                en.ev = evs_.back();
                evs_.pop_back();
                (void)hipEventRecord(en.ev, after);
            }
        }
        free_.emplace(cap, en);
    }
    uint64_t bytes() const { return bytes_; }
    void release()
    {
        (void)hipSetDevice(device);
        for (char* p : all_) (void)hipFree(p);
        for (auto& kv : free_)
            if (kv.second.ev) (void)hipEventDestroy(kv.second.ev);
        for (hipEvent_t ev : evs_) (void)hipEventDestroy(ev);
        all_.clear();
        free_.clear();
        evs_.clear();
        bytes_ = 0;
    }

private:
    struct Entry {
        char* p;
        hipEvent_t ev;
        hipStream_t st;   // the stream the event was recorded on
    };
    std::mutex m_;
    std::multimap<uint64_t, Entry> free_;
    std::vector<char*> all_;
    std::vector<hipEvent_t> evs_;
    uint64_t bytes_ = 0;
};

struct ChunkRec {
    uint64_t off = 0, len = 0;       // input bytes (host / file / device text sources)
    uint64_t site0 = 0, nsites = 0;  // synthetic sources: sites [site0, site0 + nsites)
    int dev = 0;
    uint64_t parsed = 0;             // sites found by the index
    char* held = nullptr;            // CSV records formatted in pass 1 (device)
    uint64_t held_cap = 0, held_len = 0;
    char* kept = nullptr;            // text kept for pass 2 (device)
    uint64_t kept_cap = 0, kept_len = 0;
    char* pre = nullptr;             // Lynch paths: the pass-1 parse (line offsets, counts, formatter
    uint64_t pre_cap = 0;            // header pairs: n x 28 B) kept for pass 2, which skips index + parse
    uint64_t err = ~0ull;            // min(offset * 8 + kind) of the chunk's malformed lines
    const char* host = nullptr;      // its records in the host arena (host_hold_bytes), or null
    uint64_t host_len = 0;
    bool host1 = false;              // copied there during pass 1 (the emit only writes them)
    bool sunk = false;               // device sink: formatted in pass 1 and dropped (held_len bytes)
    // BGZF sources: off / len are the compressed bytes uploaded (whole members); the chunk's lines are the
    // inflated bytes [toff, toff + tlen), which start `toff - toff(member zb0)` bytes into its first member
    uint64_t toff = 0, tlen = 0;
    uint64_t zb0 = 0, znb = 0;       // its members [zb0, zb0 + znb) of the index
    uint64_t share = 0;              // the bytes at the end of [off, off + len) that the next chunk uploads too
    uint64_t zbad = ~0ull;           // the compressed offset of its first bad member
    uint64_t kept_head = 0;          // the kept text starts there in `kept`
    // a context (sid_opts.context): the chunk's descriptor, read back with its byte count, and the bytes it
    // formatted (its forced edge records included; what the stitch keeps of them is decided at the emit)
    sid_cx_desc cx{};
    uint64_t cx_total = 0;
    // the windowed summary (sid_opts.window): the chunk's rows, read back with its byte count by the pass
    // that formats it -- once, whichever pass and path that is
    sid_win_chunk win;
    // the depth histogram (sid_engine_set_depth_hist): the chunk's rows sorted by depth, read back likewise
    std::vector<sid_dh_row> dh;
    // the region rows (sid_engine_set_region_stats): the chunk's touched intervals, checked, read back likewise
    std::vector<sid_rs_row> rs;
    // the strip crew (sid_engine_cfg.strip): the pieces the upload put together, in device order -- `dev`
    // bytes on the device that stand for `raw` input bytes (stripped: by sid_strip_lines, else the same
    // bytes); empty: the chunk went up as it is.  Read only to map a parse error's offset back
    struct StripSeg {
        uint64_t dev, raw;
        bool stripped;
    };
    std::vector<StripSeg> smap;
};

enum SrcKind { SRC_NONE, SRC_HOST, SRC_FILE, SRC_DEVICE, SRC_SYNTH_HOST, SRC_SYNTH_DEVICE, SRC_BGZF, SRC_BGZF_FILE };
// BGZF input (host memory / a file's mapping): the compressed bytes move as the text of SRC_HOST / SRC_FILE does
inline bool src_bgzf(int s) { return s == SRC_BGZF || s == SRC_BGZF_FILE; }
inline bool src_host(int s) { return s == SRC_HOST || s == SRC_BGZF; }
inline bool src_file(int s) { return s == SRC_FILE || s == SRC_BGZF_FILE; }
// a BGZF chunk's text buffer: a member's worth in front of the first line (the chunk's first member is
// written whole, its leading bytes -- the previous chunk's lines -- at negative offsets) and behind the
// last (the last member's trailing bytes, the next chunk's lines)
constexpr uint64_t ZHEAD = 65536;

// sid_chunk_ws::win_eager: four words of counts, the first rows, the first name bytes
constexpr size_t WIN_H_ROWS = 32, WIN_H_NAMES = WIN_H_ROWS + SID_WIN_EAGER_ROWS * sizeof(sid_win_row);
constexpr size_t WIN_H_BYTES = WIN_H_NAMES + SID_WIN_EAGER_NAMES;
static_assert(WIN_H_BYTES == SID_WIN_EAGER_BYTES, "the device's packed block");

struct Loaded {
    uint64_t j = 0;
    int kind = 0;            // 0 = text in a ring slot / kept buffer / device source, 1 = held records
    int slot = -1;           // ring slot, or -1
    const char* base = nullptr;
    uint64_t c0 = 0, c1 = 0;
    hipEvent_t ev = nullptr; // upload done (slot only)
    // the stripped part of the text (the strip crew): its lines and bytes, the densest the tiles will see
    uint64_t lines = 0, lbytes = 0;
};

struct OutItem {
    uint64_t j = 0;
    char* buf = nullptr;
    uint64_t cap = 0, len = 0;
    hipEvent_t ev = nullptr;  // records written (null: already complete)
    bool pooled = true;
};

struct Piece {
    uint64_t j = 0;
    int ps = -1;              // pinned slot, -1: no bytes
    uint64_t len = 0;
    bool last = false;
    char* buf = nullptr;      // the chunk's device CSV buffer, returned after the last piece
    uint64_t cap = 0;
    const char* host = nullptr;  // the whole chunk copied into the host arena instead (ps = -1)
    hipEvent_t hev = nullptr;    // that copy done
};

struct Slot {
    char* text = nullptr;
    uint64_t cap = 0;
    hipEvent_t ev_up = nullptr;    // upload done
    hipEvent_t ev_free = nullptr;  // last read of the text done
    bool used = false;
};

struct Dev {
    int index = 0, device = 0;
    // host placement (sid_engine_placement): the CPUs local to the GPU's PCI
    // device within the process's own, and its NUMA node
    cpu_set_t cpus;
    int ncpus = 0, first_cpu = -1, numa_node = -1;
    char pci[16] = {0};
    sid_ctx* ctx = nullptr;
    hipStream_t s_up = nullptr, s_comp = nullptr, s_d2h = nullptr;
    std::vector<Slot> slots;
    Chan<int> free_slots;
    Chan<Loaded> loaded;
    Chan<OutItem> drain_q;
    Chan<Piece> out_q;
    Chan<int> free_pinned;
    std::vector<char*> pinned;
    std::vector<hipEvent_t> pinned_ev;
    uint64_t pinned_cap = 0;
    sid_chunk_ws ws;
    uint64_t* h_small = nullptr;   // pinned, 16 words: [0] sites [4] error key [6..7] generator [8..11] formatter
    sid_cx_desc* h_cx = nullptr;   // pinned: the chunk's context descriptor, copied back beside the formatter's words
    // BGZF sources: the chunk's compressed bytes, member table, status words and result on the device (one
    // buffer: the uploader waits for each chunk's inflate before it loads the next), and the table's
    // pinned staging ([0] the result read back, from [16] the table)
    char* zbuf = nullptr;
    uint64_t zcap = 0;
    char* ztab_h = nullptr;
    uint64_t ztab_cap = 0;
    DevPool pool;
    // hold arena: the records formatted in pass 1, packed one after another
    // in segments of HBM kept across runs; a chunk reserves its upper bound
    // and commits its exact bytes
    std::vector<std::pair<char*, uint64_t>> arena;
    size_t arena_seg = 0;
    uint64_t arena_off = 0;
    // `left`: what the hold budget still allows (a new segment is not made
    // larger than that, nor than 4 GiB, nor smaller than `need`); null when
    // the HBM is not there (the caller formats the chunk in pass 2 instead)
    char* arena_reserve(uint64_t need, uint64_t left)
    {
        while (arena_seg < arena.size() && arena_off + need > arena[arena_seg].second) ++arena_seg, arena_off = 0;
        if (arena_seg == arena.size()) {
            const uint64_t want = std::min<uint64_t>(4ull << 30, std::max(need, left));
            const uint64_t c = (std::max(need, want) + (2u << 20) - 1) & ~(uint64_t)((2u << 20) - 1);
            char* p = nullptr;
            if (hipMalloc(&p, c) != hipSuccess) {
                (void)hipGetLastError();   // not an error: the chunk is formatted in pass 2 (see DevPool::get)
                return nullptr;
            }
            arena.push_back({p, c});
            arena_off = 0;
        }
        return arena[arena_seg].first + arena_off;
    }
    void arena_commit(uint64_t bytes) { arena_off += (bytes + 255) & ~(uint64_t)255; }
    uint64_t arena_bytes() const
    {
        uint64_t b = 0;
        for (auto& a : arena) b += a.second;
        return b;
    }
    // host arena (sid_engine_cfg.host_hold_bytes): pinned host memory, made
    // once and reused by every run, that receives the records D2H -- in pass
    // 1 while later chunks upload (full duplex), in pass 2 instead of the
    // pinned ring; bump-allocated, reset by every ingest
    char* hh = nullptr;
    uint64_t hh_cap = 0, hh_off = 0;
    bool hh_full = false;
    bool hh_alloc(uint64_t bytes)
    {
        if (hipHostMalloc((void**)&hh, bytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            hh = nullptr;
            return false;
        }
        hh_cap = bytes;
        return true;
    }
    void hh_free()
    {
        if (hh) (void)hipHostFree(hh);
        hh = nullptr;
        hh_cap = 0;
    }
    char* hh_take(uint64_t bytes)
    {
        if (!hh || hh_off + bytes > hh_cap) return nullptr;
        char* p = hh + hh_off;
        hh_off += (bytes + 255) & ~(uint64_t)255;
        return p;
    }
    // the tile parse (sid_chunk_tile_local): its slots per tile for the next
    // chunk (tile_next / tile_over), its shape (a quad of lanes per line for
    // lines over 256 B on average), and whether it takes the lines at all (at
    // most SID_TILE_CAP_MAX a tile)
    uint32_t tile_cap = 288;
    bool tile_quad = false;
    bool tile_ok = true;
    // slots per tile for at most `lines` lines a tile: multiples of 16, up to
    // the shape's list (a quad tile of lines too short for its list: the lane
    // shape instead)
    uint64_t tile_hi = 0;   // the lines a tile should have room for (a decaying maximum over chunks)
    void tile_set(uint64_t lines, bool quad)
    {
        if (quad && lines > SID_TILE_CAP_MAX_QUAD) {
            quad = false;
            lines = lines * sid_tile_unit(false) / sid_tile_unit(true) + 1;
        }
        tile_quad = quad;
        tile_hi = lines;
        tile_cap = (uint32_t)std::min<uint64_t>(quad ? SID_TILE_CAP_MAX_QUAD : SID_TILE_CAP_MAX,
                                                std::max<uint64_t>(SID_TILE_CAP_MIN, (lines + 15) & ~15ull));
    }
    // after a tiled chunk of n sites over `bytes` of text whose tiles had at
    // most maxl lines: the next chunk's shape (a quad of lanes per line over
    // 256 B a line) and slots (the same shape: maxl, a thirty-second and 2 on
    // top, or the room recent chunks needed, less a sixty-fourth a chunk --
    // chunks whose fullest tiles alternate would otherwise overflow every
    // other chunk; a new shape: from this chunk's lines per byte, a quarter on
    // top)
    void tile_next(uint64_t maxl, uint64_t n, uint64_t bytes, bool quad)
    {
        const bool q2 = bytes > 256 * n;
        if (q2 == quad)
            tile_set(std::max<uint64_t>(maxl + maxl / 32 + 2, tile_hi - tile_hi / 64), q2);
        else
            tile_set((uint64_t)((double)n * sid_tile_unit(q2) / (double)std::max<uint64_t>(1, bytes) * 1.25) + 1, q2);
    }
    // before a chunk with `lines` lines in `bytes` of stripped text (the strip crew: about 1.6 times the
    // lines per byte of the text the slots were learned on) is parsed: the slots that density needs, a
    // quarter on top as for a new shape, when they exceed the current ones -- or its shape, when that differs
    void tile_ahead(uint64_t lines, uint64_t bytes)
    {
        if (!lines || !bytes || !tile_ok) return;
        const bool q2 = bytes > 256 * lines;
        const uint64_t per = (uint64_t)((double)lines * sid_tile_unit(q2) / (double)bytes * 1.25) + 1;
        if (q2 != tile_quad) tile_set(per, q2);
        else if (((per + 15) & ~15ull) > tile_cap) tile_set(std::max(per, tile_hi), q2);
    }
    // a tile had more lines than slots (the chunk goes the two-pass way); the
    // tile parse stays off while no shape has room for them: judged in the
    // units of the shape tile_set chose (a quad tile's lines counted in lane
    // tiles when it switched to the lane shape)
    void tile_over(uint64_t maxl, bool quad)
    {
        tile_set(maxl + maxl / 32 + 2, quad);
        const uint64_t need = quad && !tile_quad ? maxl * sid_tile_unit(false) / sid_tile_unit(true) + 1 : maxl;
        tile_ok = need <= (tile_quad ? SID_TILE_CAP_MAX_QUAD : SID_TILE_CAP_MAX);
    }
    // the tile parse off (a run of tiny lines): after a two-pass chunk of n
    // sites over `bytes` whose lines per byte leave a lane tile half its
    // largest list, on again with that chunk's density (a quarter on top);
    // a tile of tiny lines in it overflows and turns it off again
    void tile_retry(uint64_t n, uint64_t bytes)
    {
        const uint64_t per = (uint64_t)((double)n * sid_tile_unit(false) / (double)std::max<uint64_t>(1, bytes) * 1.25) + 1;
        if (tile_ok || 2 * per > SID_TILE_CAP_MAX) return;
        tile_hi = 0;
        tile_set(per, false);
        tile_ok = true;
    }
    // a new run: a device the last run left with the tile parse off starts
    // from the defaults (a run that kept it on keeps its shape and slots, the
    // next run's likely fit)
    void tile_reset()
    {
        if (tile_ok) return;
        tile_cap = 288;
        tile_quad = false;
        tile_hi = 0;
        tile_ok = true;
    }
    // the strip crew's pinned staging (sid_engine_cfg.strip): a ring of chunk-sized buffers, made once
    // and reused by every run, and per buffer the event of the last copies out of it
    static constexpr int STRIP_RING = 3;
    char* sbuf[STRIP_RING] = {nullptr, nullptr, nullptr};
    hipEvent_t sev[STRIP_RING] = {nullptr, nullptr, nullptr};
    uint64_t scap = 0;
    uint64_t hold_budget = 0, retain_budget = 0;
    std::atomic<uint64_t> hold_used{0}, retain_used{0};
    std::atomic<bool> hold_full{false};
    // the ingest's host-to-device copies, timed on the upload stream (pairs
    // of timing events, summed after the ingest's sync)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> h2d_pending;
    std::vector<hipEvent_t> h2d_free;
    uint64_t h2d_bytes = 0;
    uint64_t tiled = 0, tile_overflows = 0, tile_over_queued = 0;   // this run's chunks (the device's compute thread)
    hipEvent_t h2d_event()
    {
        hipEvent_t ev = nullptr;
        if (!h2d_free.empty()) {
            ev = h2d_free.back();
            h2d_free.pop_back();
        } else if (hipEventCreate(&ev) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        return ev;
    }
    // device time of the uploads timed since the last call (the stream
    // drained): each uploader's span, first copy's start to last copy's end
    double h2d_collect()
    {
        double s = 0;
        for (auto& pr : h2d_pending) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) s += ms * 1e-3;
            h2d_free.push_back(pr.first);
            h2d_free.push_back(pr.second);
        }
        (void)hipGetLastError();
        h2d_pending.clear();
        return s;
    }
    std::mutex ev_m;
    std::vector<hipEvent_t> ev_cache;   // events marking a chunk's records written (compute -> drain)
    // sid_engine_profile: (stage, start, end) per stage and chunk, read after a sync
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> prof_pending;
    std::vector<hipEvent_t> prof_free;
    uint64_t prof_chunks = 0;
    hipEvent_t prof_begin(bool on)
    {
        if (!on) return nullptr;
        hipEvent_t ev = nullptr;
        if (!prof_free.empty()) {
            ev = prof_free.back();
            prof_free.pop_back();
        } else if (hipEventCreate(&ev) != hipSuccess) {
            return nullptr;
        }
        (void)hipEventRecord(ev, s_comp);
        return ev;
    }
    void prof_end(int stage, hipEvent_t start)
    {
        if (!start) return;
        hipEvent_t ev = prof_begin(true);
        if (ev) prof_pending.push_back({stage, {start, ev}});
    }
    hipEvent_t take_event()
    {
        std::lock_guard<std::mutex> l(ev_m);
        hipEvent_t ev = nullptr;
        if (!ev_cache.empty()) {
            ev = ev_cache.back();
            ev_cache.pop_back();
        } else if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
            ev = nullptr;
        }
        return ev;
    }
    void give_event(hipEvent_t ev)
    {
        std::lock_guard<std::mutex> l(ev_m);
        ev_cache.push_back(ev);
    }
};

// The CPUs of a sysfs cpulist ("0-15,128-143") within `allowed`
int parse_cpulist(const char* txt, const cpu_set_t& allowed, cpu_set_t* out, int* first)
{
    CPU_ZERO(out);
    int n = 0;
    *first = -1;
    const char* p = txt;
    while (*p) {
        char* q = nullptr;
        const long lo = std::strtol(p, &q, 10);
        if (q == p) break;
        long hi = lo;
        p = q;
        if (*p == '-') {
            hi = std::strtol(p + 1, &q, 10);
            p = q;
        }
        for (long c = lo; c <= hi && c < CPU_SETSIZE; ++c)
            if (c >= 0 && CPU_ISSET(c, &allowed) && !CPU_ISSET(c, out)) {
                CPU_SET(c, out);
                if (*first < 0 || c < *first) *first = (int)c;
                ++n;
            }
        while (*p == ',' || *p == '\n' || *p == ' ') ++p;
    }
    return n;
}

// d's GPU: its PCI bus id, NUMA node and local CPUs (sysfs), kept for
// binding when they are a proper subset of the process's CPUs
void find_placement(Dev& d)
{
    CPU_ZERO(&d.cpus);
    if (hipDeviceGetPCIBusId(d.pci, sizeof d.pci, d.device) != hipSuccess) {
        (void)hipGetLastError();
        d.pci[0] = 0;
        return;
    }
    for (char* c = d.pci; *c; ++c) *c = (char)std::tolower((unsigned char)*c);
    char path[128], buf[4096];
    std::snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", d.pci);
    if (FILE* f = std::fopen(path, "r")) {
        if (std::fscanf(f, "%d", &d.numa_node) != 1) d.numa_node = -1;
        std::fclose(f);
    }
    std::snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/local_cpulist", d.pci);
    FILE* f = std::fopen(path, "r");
    if (!f) return;
    const size_t m = std::fread(buf, 1, sizeof buf - 1, f);
    std::fclose(f);
    buf[m] = 0;
    cpu_set_t allowed;
    if (sched_getaffinity(0, sizeof allowed, &allowed) != 0) return;
    cpu_set_t mine;
    int first = -1;
    const int n = parse_cpulist(buf, allowed, &mine, &first);
    if (n == 0 || n == CPU_COUNT(&allowed)) return;   // nothing to choose
    d.cpus = mine;
    d.ncpus = n;
    d.first_cpu = first;
}

// the calling thread onto d's CPUs (no-op when not bound)
void bind_thread(const Dev& d)
{
    if (d.ncpus > 0) (void)pthread_setaffinity_np(pthread_self(), sizeof d.cpus, &d.cpus);
}

// NUMA node of the page holding p (-1: unknown)
int page_node(const void* p)
{
    if (!p) return -1;
    int node = -1;
    // get_mempolicy(&node, NULL, 0, p, MPOL_F_NODE | MPOL_F_ADDR)
    if (syscall(SYS_get_mempolicy, &node, nullptr, 0ul, p, 1ul | 2ul) != 0) return -1;
    return node;
}

// f() on a thread bound to d's CPUs (pinned host buffers then come from the
// GPU's NUMA node: the pages are allocated by the thread that pins them)
template <class F>
void on_node(const Dev& d, F f)
{
    if (d.ncpus == 0) return f();
    std::thread t([&] {
        bind_thread(d);
        f();
    });
    t.join();
}

// The engine's run threads, kept across runs (spawning a run's uploader and
// compute threads took 0.08-0.15 ms of every run, the device idle behind
// them): run() gives each task of a batch a thread of its own (uploader and
// compute wait on each other through the queues) and returns when all are
// done.  A task starts with the affinity its thread was created with (the
// caller's), as a thread spawned for it would.
class Crew {
  public:
    Crew() = default;
    Crew(const Crew&) = delete;
    Crew& operator=(const Crew&) = delete;
    ~Crew()
    {
        {
            std::lock_guard<std::mutex> l(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    // the batch started (one batch at a time); wait() returns when it is done
    void start(std::vector<std::function<void()>>& fs)
    {
        std::lock_guard<std::mutex> l(m_);
        if (tasks_.size() < fs.size()) tasks_.resize(fs.size());
        while (th_.size() < fs.size()) {
            const size_t k = th_.size();
            th_.emplace_back([this, k] { loop(k); });
        }
        for (size_t k = 0; k < fs.size(); ++k) tasks_[k] = std::move(fs[k]);
        pending_ = fs.size();
        cv_.notify_all();
    }
    void wait()
    {
        std::unique_lock<std::mutex> l(m_);
        done_.wait(l, [&] { return pending_ == 0; });
    }
    void run(std::vector<std::function<void()>>& fs)
    {
        start(fs);
        wait();
    }

  private:
    void loop(size_t k)
    {
        cpu_set_t base;
        const bool aff = pthread_getaffinity_np(pthread_self(), sizeof base, &base) == 0;
        std::unique_lock<std::mutex> l(m_);
        for (;;) {
            cv_.wait(l, [&] { return stop_ || tasks_[k] != nullptr; });
            if (stop_) return;
            std::function<void()> f = std::move(tasks_[k]);
            tasks_[k] = nullptr;
            l.unlock();
            if (aff) (void)pthread_setaffinity_np(pthread_self(), sizeof base, &base);
            f();
            l.lock();
            if (--pending_ == 0) done_.notify_all();
        }
    }
    std::mutex m_;
    std::condition_variable cv_, done_;
    std::vector<std::thread> th_;
    std::vector<std::function<void()>> tasks_;   // (resized under m_ only, before a worker can see its slot)
    size_t pending_ = 0;
    bool stop_ = false;
};

// One device's strip crew for one ingest (sid_engine_cfg.strip).  Job k is the k-th chunk
// of the device's uploader.  Crew thread t strips region t -- a line-aligned T-th -- of job k into its
// part of staging buffer k % STRIP_RING, publishing after every STRIP_STEP input bytes how far it is
// (whole lines, their bytes visible); the uploader, when it holds a device buffer for the chunk, takes
// every region as far as it got -- the stripped bytes from the staging, the rest of the region from the
// source -- and the crew goes on to job k + 1.  A buffer is written again once the copies out of it
// are done (the leader, thread 0, waits for their event).
constexpr uint64_t STRIP_STEP = 128u << 10;
struct StripProg {
    std::mutex m;
    uint64_t in_done = 0, out_done = 0, lines = 0;
    bool taken = false;   // the uploader has read it: the thread stops
};
struct StripJob {
    std::unique_ptr<StripProg[]> P;   // per crew thread
    std::vector<uint64_t> cut;        // the regions' bounds in the chunk, T + 1 of them
};
struct StripRun {
    int T = 0;
    int mode = 0;   // sid_engine_cfg.strip: 0 what is ready in time, 1 every chunk whole, 2 every other one
    std::vector<StripJob> jobs;
    std::mutex m;
    std::condition_variable cv;
    std::vector<int> fin;   // per job: the threads that have left it
    uint64_t decided = 0;   // jobs [0, decided) were taken by the uploader
    uint64_t ready = 0;     // jobs [0, ready) have their staging buffer free (the leader)
    bool stop = false;      // the uploader is done
    bool sev_used[Dev::STRIP_RING] = {false, false, false};   // the buffer's event was recorded in this run
    bool wanted(uint64_t k) const { return mode != 2 || !(k & 1); }
    // region t's place in a staging buffer: 64-B aligned, behind region t - 1's bytes
    uint64_t place(const StripJob& J, int t) const { return (J.cut[t] + 64 * (uint64_t)t + 63) & ~(uint64_t)63; }
};

}  // namespace

struct sid_engine {
    sid_opts opts{};
    sid_engine_cfg cfg{};
    std::vector<std::unique_ptr<Dev>> devs;
    // source
    int src = SRC_NONE;
    const char* text = nullptr;     // SRC_HOST / SRC_FILE (mapping) / SRC_DEVICE; SRC_BGZF*: the compressed bytes
    sid_bgzf* zidx = nullptr;       // SRC_BGZF*: the member index
    std::atomic<uint64_t> z_bytes{0}, z_blocks{0};   // compressed bytes / members uploaded in pass 1
    uint64_t text_len = 0;
    bool reg_upload = false;        // SRC_HOST / SRC_FILE pageable: chunks registered for DMA (upload_register)
    void* map = nullptr;
    uint64_t map_len = 0, map_skew = 0;
    uint64_t synth_seed = 0, synth_first = 0, synth_n = 0, synth_spc = 0, synth_per = 0;
    double synth_depth = 30.0;
    std::vector<uint64_t> synth_cdf;
    uint64_t* d_cdf = nullptr;       // on the first device (SRC_SYNTH_DEVICE)
    std::vector<uint64_t*> d_cdf_dev;
    std::vector<sid_synth_gen_ws> gen_ws;
    std::vector<ChunkRec> recs;
    // run state
    bool lynch = false, quality = false, ingested = false, estimated = false;
    bool hist_merged = false;        // the pipelines' Lynch histograms hold the merged table
    const char* conf_type = "p_value";
    std::atomic<int> rc{SID_OK};
    std::atomic<uint64_t> first_err{UINT64_MAX};
    std::atomic<uint64_t> reloaded{0};
    std::atomic<uint64_t> sink_bytes{0};   // device sink: CSV bytes formatted and dropped
    // SID_ENGINE_TIMING: host time (ns) spent in compute-stream syncs and in
    // the writer's waits for D2H pieces, printed per phase
    std::atomic<uint64_t> t_comp_sync{0}, t_write_wait{0};
    std::atomic<uint64_t> reg_chunks{0};   // chunks uploaded from registered pages (upload_register)
    std::atomic<uint64_t> t_register{0};   // ns in hipHostRegister / hipHostUnregister (the uploaders)
    // the strip crews (sid_engine_cfg.strip): threads per device (0: off), whether the source is host
    // memory pinned already, this run's crews, its chunks uploaded with stripped bytes, the input bytes
    // not uploaded, and the crews' busy time (ns in sid_strip_stream, summed over the threads)
    int strip_T = 0;
    bool src_pinned = false;
    std::vector<std::unique_ptr<StripRun>> strip_runs;
    std::atomic<uint64_t> strip_chunks{0}, strip_bytes{0}, t_strip{0};
    std::atomic<uint64_t> t_strip_min{UINT64_MAX}, t_strip_max{0};   // ... and the least and most busy thread's
    uint64_t last_h2d_bytes = 0;   // the last ingest's sid_run_stats.h2d_bytes (SID_ENGINE_TIMING)
    // host-generated input: pinned buffers
    std::vector<char*> gen_buf;
    std::vector<uint64_t> gen_cap;
    std::vector<hipEvent_t> gen_ev;   // H2D of the buffer done (recorded by the uploader)
    std::vector<int> gen_dev;         // device whose stream recorded gen_ev
    uint64_t per_chunk_cap = 0;
    sid_estimate est{};
    int cx_n = 0;                    // the context in effect (sid_ctx::cx_n: 0 without a selection)
    bool cx_on = false;              // ... and whether its route is (sid_ctx::cx_on)
    sid_win_table win;               // sid_opts.window: the run's rows, stitched by the emit
    bool win_ready = false;
    bool depth_hist = false;         // sid_engine_set_depth_hist
    std::vector<sid_depth_row> dh;   // ... the run's rows, the chunks' summed by the emit
    bool dh_ready = false;
    bool region_stats = false;       // sid_engine_set_region_stats
    sid_region_row* rs = nullptr;    // ... the run's rows, the chunks' summed by the emit (sid_rs_export)
    size_t rs_n = 0;
    bool rs_ready = false;
    bool prof = false;
    double prof_ms[6] = {0, 0, 0, 0, 0, 0};   // sid_engine_prof order: index parse call hist fmt_len fmt_write
    uint64_t prof_chunks = 0;
    Crew crew;   // (last: its threads joined first when the engine is deleted)
};

namespace {

void close_all(sid_engine* e)
{
    for (auto& d : e->devs) {
        d->free_slots.close();
        d->loaded.close();
        d->drain_q.close();
        d->out_q.close();
        d->free_pinned.close();
    }
}

// the first failure wins; every queue closes so no thread waits on a peer
// that has stopped
void fail(sid_engine* e, int rc)
{
    int ok = SID_OK;
    e->rc.compare_exchange_strong(ok, rc);
    close_all(e);
}

int hipfail(sid_engine* e, hipError_t x)
{
    if (x == hipSuccess) return SID_OK;
    const int rc = sid_set_hip_error(x);
    fail(e, rc);
    return rc;
}

// default chunk sizes: input that crosses PCIe in 128 MiB pieces (the pipeline
// fills and drains in a few ms); text already in HBM, or generated there, in
// larger ones (every chunk costs a few fixed launches and two host round
// trips; the workspace is a few hundred MB per GiB of text)
const uint64_t CHUNK_HOST = 128ull << 20;
const uint64_t CHUNK_DEVICE = 4000ull << 20;   // C2 2.95-2.97 vs 2.97-2.99 ms with 2 GiB, C5 13.7 vs 14.2 ms (round 5)
const uint64_t CHUNK_SYNTH = 512ull << 20;

uint64_t chunk_bytes(const sid_engine* e)
{
    // (32-bit line offsets: a chunk spans less than 4 GiB, sid_off_t)
    if (e->cfg.chunk_bytes) return std::min<uint64_t>(e->cfg.chunk_bytes, SID_CHUNK_MAX - (64ull << 20));
    return e->src == SRC_DEVICE ? CHUNK_DEVICE : e->src == SRC_SYNTH_DEVICE ? CHUNK_SYNTH : CHUNK_HOST;
}

// first line start at or after c (one past the next '\n')
uint64_t next_line_start(const char* t, uint64_t len, uint64_t c)
{
    if (c == 0 || c >= len) return std::min(c, len);
    const char* nl = (const char*)std::memchr(t + c - 1, '\n', len - c + 1);
    return nl ? (uint64_t)(nl - t) + 1 : len;
}

void split_host_text(sid_engine* e, const char* t, uint64_t len)
{
    const uint64_t C = chunk_bytes(e);
    e->recs.clear();
    uint64_t at = 0;
    while (at < len) {
        // the last chunks' work (compute, then their records' copies back)
        // runs after the last upload: the last two chunks' worth of text is
        // cut in halves down to 8-16 MiB, so each chunk's D2H (~0.6 of its
        // upload's time) runs under the uploads still to come, and what is
        // left after the last upload is one small chunk's
        const uint64_t rem = len - at;
        const uint64_t want = rem <= 2 * C && rem > (16ull << 20) ? std::min(C, rem / 2) : C;
        uint64_t end = next_line_start(t, len, std::max(at + 1, std::min(len, at + want)));
        if (end <= at) end = len;
        ChunkRec r;
        r.off = at;
        r.len = end - at;
        e->recs.push_back(r);
        at = end;
    }
}

// ------------------------------------------------------------- generator --
// the synthetic text of sites [first, first + n) into dst (cap bytes); the
// same bytes as sid_synth_text (capi.cpp), without intermediate strings.
// Returns the length, or UINT64_MAX when it does not fit.
uint64_t synth_host(const std::vector<uint64_t>& cdf, uint64_t seed, uint64_t first, uint64_t n, uint64_t spc,
                    char* dst, uint64_t cap)
{
    static const char UP[] = "ACGT", LO[] = "acgt";
    const uint32_t k = (uint32_t)cdf.size();
    char* o = dst;
    char* const end = dst + cap;
    auto put_u = [&](uint64_t v) {
        char tmp[24];
        int m = 0;
        do {
            tmp[m++] = (char)('0' + v % 10);
            v /= 10;
        } while (v);
        while (m) *o++ = tmp[--m];
    };
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t site = first + i;
        const uint64_t chrom = spc ? site / spc + 1 : 1;
        const uint64_t pos = spc ? site % spc + 1 : site + 1;
        sid_synth_site s = sid_synth_site_header(seed, site, cdf.data(), k);
        // worst case of this line: names and numbers (64) + 4 bytes per read
        if ((uint64_t)(end - o) < 64 + 5ull * s.depth) return UINT64_MAX;
        *o++ = 'c';
        *o++ = 'h';
        *o++ = 'r';
        put_u(chrom);
        *o++ = '\t';
        put_u(pos);
        *o++ = '\t';
        *o++ = UP[s.ref];
        *o++ = '\t';
        put_u(s.depth);
        *o++ = '\t';
        if (s.depth == 0) {
            *o++ = '*';
            *o++ = '\t';
            *o++ = '*';
            *o++ = '\n';
            continue;
        }
        char* q = o + 4 * s.depth;   // qualities after the bases: written in one walk
        char* qs = q;
        for (uint32_t r = 0; r < s.depth; ++r) {
            uint32_t strand;
            const uint32_t b = sid_synth_read_base(&s, r, &strand);
            int st, en;
            uint32_t ql;
            sid_synth_read_marks(&s, r, &st, &en, &ql);
            if (st) {
                *o++ = '^';
                *o++ = ']';
            }
            *o++ = b == s.ref ? (strand ? '.' : ',') : (strand ? UP[b] : LO[b]);
            if (en) *o++ = '$';
            *q++ = (char)('!' + ql);
        }
        *o++ = '\t';
        std::memmove(o, qs, s.depth);
        o += s.depth;
        *o++ = '\n';
    }
    return (uint64_t)(o - dst);
}

// The strip crew's threads per pipeline (sid_engine_cfg.strip; 0: no crew): host_threads when set, else
// the CPUs the process may use -- the smaller of its affinity mask and its cgroup's cpu.max, shared among
// LOCAL_WORLD_SIZE ranks and this engine's pipelines -- less two (the uploader, the compute thread), at
// most 14.  Fewer than two: off.  SID_STRIP=0: off.
int strip_threads(const sid_engine_cfg& cfg, int pipelines)
{
    if (cfg.strip < 0) return 0;
    if (const char* v = std::getenv("SID_STRIP"))
        if (std::atoi(v) == 0) return 0;
    int T = cfg.host_threads;
    if (T <= 0) {
        cpu_set_t allowed;
        long n = sched_getaffinity(0, sizeof allowed, &allowed) == 0 ? CPU_COUNT(&allowed) : 1;
        if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
            long long quota = 0, period = 0;
            if (std::fscanf(f, "%lld %lld", &quota, &period) == 2 && quota > 0 && period > 0)
                n = std::min<long>(n, (long)std::max<long long>(1, quota / period));
            std::fclose(f);
        }
        if (const char* w = std::getenv("LOCAL_WORLD_SIZE"))
            if (std::atoi(w) > 1) n /= std::atoi(w);
        n /= std::max(1, pipelines);
        T = (int)std::min<long>(14, n - 2);
    }
    return T >= 2 ? std::min(T, 64) : 0;
}

}  // namespace

// ================================================================= C ABI ==
extern "C" void sid_engine_cfg_default(sid_engine_cfg* c)
{
    if (!c) return;
    std::memset(c, 0, sizeof *c);
}

extern "C" int sid_engine_create(const sid_opts* opts, const sid_engine_cfg* cfg, sid_engine** out)
{
    if (!out) return SID_EINVAL;
    *out = nullptr;
    if (opts && (opts->select < SID_SELECT_ALL || opts->select > SID_SELECT_HOM)) return SID_EINVAL;
    if (opts && (opts->context < 0 || opts->context > SID_CONTEXT_MAX)) return SID_EINVAL;
    if (opts && opts->window < 0) return SID_EINVAL;
    int nvis = 0;
    if (hipGetDeviceCount(&nvis) != hipSuccess || nvis <= 0) return SID_EHIP;
    sid_engine* e = new sid_engine();
    if (opts) e->opts = *opts; else sid_opts_default(&e->opts);
    if (cfg) e->cfg = *cfg; else sid_engine_cfg_default(&e->cfg);
    const int G = e->cfg.devices > 0 ? e->cfg.devices : nvis;
    const int lanes = std::max(1, e->cfg.lanes);
    const int D = G * lanes;   // pipelines
    const int R = e->cfg.slots > 0 ? e->cfg.slots : 3;
    for (int i = 0; i < D; ++i) {
        auto d = std::make_unique<Dev>();
        d->index = i;
        d->device = (e->cfg.first_device + i / lanes) % nvis;
        d->pool.device = d->device;
        e->devs.push_back(std::move(d));
    }
    // every pipeline's context (class tables, the first kernel launches on
    // its GPU), streams and events: one thread per GPU, its pipelines in
    // order -- the GPUs' start-up costs (tens of ms each) overlap instead of
    // adding up on a whole node
    std::vector<int> rcs(D, SID_OK);
    // (the streams -- a hardware queue each, ~8 ms apiece -- are created on a
    // second thread while sid_create builds the class tables)
    auto make = [&](int i) {
        Dev* d = e->devs[i].get();
        find_placement(*d);
        bind_thread(*d);   // (this GPU's start-up thread: its host allocations local to it)
        hipError_t x = hipSuccess;
        std::thread qs([&] {
            bind_thread(*d);
            x = hipSetDevice(d->device);
            if (x == hipSuccess) x = hipStreamCreateWithFlags(&d->s_up, hipStreamNonBlocking);
            if (x == hipSuccess) x = hipStreamCreateWithFlags(&d->s_comp, hipStreamNonBlocking);
            if (x == hipSuccess) x = hipStreamCreateWithFlags(&d->s_d2h, hipStreamNonBlocking);
            if (x == hipSuccess) x = hipHostMalloc((void**)&d->h_small, 128, hipHostMallocDefault);
            if (x == hipSuccess) x = hipHostMalloc((void**)&d->h_cx, sizeof(sid_cx_desc), hipHostMallocDefault);
            d->slots.resize(R);
            for (auto& s : d->slots) {
                if (x == hipSuccess) x = hipEventCreateWithFlags(&s.ev_up, hipEventDisableTiming);
                if (x == hipSuccess) x = hipEventCreateWithFlags(&s.ev_free, hipEventDisableTiming);
            }
        });
        int rc = sid_create(d->device, &e->opts, &d->ctx);
        // (the formatters that take no context, sid_chunk_fmt_len / _put: the options as the context holds them)
        if (rc == SID_OK) sid_chunk_bind_context(&d->ws, d->ctx);
        qs.join();
        if (rc == SID_OK && x != hipSuccess) rc = sid_set_hip_error(x);
        rcs[i] = rc;
    };
    auto per_gpu = [&](int g) {
        for (int i = g * lanes; i < std::min(D, (g + 1) * lanes); ++i) make(i);
    };
    {   // (each on a thread of its own: make() binds its thread to the GPU's CPUs)
        std::vector<std::thread> th;
        for (int g = 0; g < G; ++g) th.emplace_back(per_gpu, g);
        for (auto& t : th) t.join();
    }
    (void)hipSetDevice(e->devs[0]->device);
    e->opts.regions = nullptr;   // (every context holds its own copy: the caller may free the object now)
    for (int rc : rcs)
        if (rc != SID_OK) {
            sid_engine_destroy(e);
            return rc;
        }
    e->cx_n = e->devs[0]->ctx->cx_n;
    e->cx_on = e->devs[0]->ctx->cx_on;
    e->strip_T = strip_threads(e->cfg, D);
    *out = e;
    return SID_OK;
}

static void drop_source(sid_engine* e)
{
    if (e->map) munmap(e->map, e->map_len);
    e->map = nullptr;
    for (auto& r : e->recs) {
        Dev& d = *e->devs[r.dev];
        if (r.held) d.pool.put(r.held, r.held_cap, nullptr);
        if (r.kept) d.pool.put(r.kept, r.kept_cap, nullptr);
        if (r.pre) d.pool.put(r.pre, r.pre_cap, nullptr);
        r.held = r.kept = r.pre = nullptr;
    }
    e->recs.clear();
    e->win.clear();
    e->win_ready = false;
    e->dh.clear();
    e->dh_ready = false;
    sid_region_stats_free(e->rs);
    e->rs = nullptr, e->rs_n = 0;
    e->rs_ready = false;
    sid_bgzf_free(e->zidx);
    e->zidx = nullptr;
    e->src = SRC_NONE;
    e->src_pinned = false;
    e->text = nullptr;
    e->text_len = 0;
    e->ingested = e->estimated = false;
}

extern "C" int sid_engine_destroy(sid_engine* e)
{
    if (!e) return SID_OK;
    for (auto& d : e->devs) (void)hipSetDevice(d->device), (void)hipDeviceSynchronize();
    drop_source(e);
    for (auto& d : e->devs) {
        (void)hipSetDevice(d->device);
        for (auto& s : d->slots) {
            if (s.text) (void)hipFree(s.text);
            if (s.ev_up) (void)hipEventDestroy(s.ev_up);
            if (s.ev_free) (void)hipEventDestroy(s.ev_free);
        }
        for (char* p : d->pinned) (void)hipHostFree(p);
        for (char* p : d->sbuf)
            if (p) (void)hipHostFree(p);
        for (hipEvent_t ev : d->sev)
            if (ev) (void)hipEventDestroy(ev);
        d->hh_free();
        for (hipEvent_t ev : d->pinned_ev) (void)hipEventDestroy(ev);
        for (hipEvent_t ev : d->ev_cache) (void)hipEventDestroy(ev);
        for (auto& pr : d->prof_pending) (void)hipEventDestroy(pr.second.first), (void)hipEventDestroy(pr.second.second);
        for (hipEvent_t ev : d->prof_free) (void)hipEventDestroy(ev);
        for (auto& pr : d->h2d_pending) (void)hipEventDestroy(pr.first), (void)hipEventDestroy(pr.second);
        for (hipEvent_t ev : d->h2d_free) (void)hipEventDestroy(ev);
        sid_chunk_release(&d->ws);
        if (d->h_small) (void)hipHostFree(d->h_small);
        if (d->h_cx) (void)hipHostFree(d->h_cx);
        if (d->zbuf) (void)hipFree(d->zbuf);
        if (d->ztab_h) (void)hipHostFree(d->ztab_h);
        for (hipStream_t s : {d->s_up, d->s_comp, d->s_d2h})
            if (s) (void)hipStreamDestroy(s);
        d->pool.release();
        for (auto& a : d->arena) (void)hipFree(a.first);
        sid_destroy(d->ctx);
    }
    for (size_t i = 0; i < e->d_cdf_dev.size(); ++i)
        if (e->d_cdf_dev[i]) (void)hipSetDevice(e->devs[i]->device), (void)hipFree(e->d_cdf_dev[i]);
    for (size_t i = 0; i < e->gen_ws.size(); ++i) {
        (void)hipSetDevice(e->devs[i]->device);
        sid_synth_gen_release(&e->gen_ws[i]);
    }
    for (char* p : e->gen_buf) (void)hipHostFree(p);
    for (hipEvent_t ev : e->gen_ev)
        if (ev) (void)hipEventDestroy(ev);
    delete e;
    return SID_OK;
}

extern "C" int sid_engine_devices(const sid_engine* e) { return e ? (int)e->devs.size() : 0; }

extern "C" sid_ctx* sid_engine_context(sid_engine* e, int i)
{
    if (!e || i < 0 || i >= (int)e->devs.size()) return nullptr;
    return e->devs[i]->ctx;
}

// The depth bounds of every pipeline's context, and of its workspace (the
// formatters that take no context); the context's route follows where the
// bounds alone select under sid_opts.context.  Not between an ingest and its
// emit: -m local's records are formatted by then, the others' are not.
extern "C" int sid_engine_set_depth(sid_engine* e, int min, int max)
{
    if (!e) return SID_EINVAL;
    if (min < 0 || min > SID_DEPTH_MAX || (max != 0 && (max < min || max > SID_DEPTH_MAX))) return SID_EINVAL;
    if (e->ingested) return SID_ESTATE;
    for (auto& d : e->devs) {
        const int rc = sid_set_depth(d->ctx, min, max);
        if (rc != SID_OK) return rc;
        sid_chunk_bind_context(&d->ws, d->ctx);
    }
    e->cx_n = e->devs[0]->ctx->cx_n;
    e->cx_on = e->devs[0]->ctx->cx_on;
    return SID_OK;
}

// The record format of every pipeline's context and workspace (sid.h
// Conventions, "VCF"), under sid_engine_set_depth's state rules: -m local's
// records are formatted during the ingest.  The workspaces keep the sites'
// reference bytes from their next reservation on.
extern "C" int sid_engine_set_format(sid_engine* e, int format)
{
    if (!e || (format != SID_FORMAT_CSV && format != SID_FORMAT_VCF)) return SID_EINVAL;
    if (e->ingested) return SID_ESTATE;
    for (auto& d : e->devs) {
        const int rc = sid_set_format(d->ctx, format);
        if (rc != SID_OK) return rc;
        sid_chunk_bind_context(&d->ws, d->ctx);
    }
    return SID_OK;
}

extern "C" int sid_engine_placement(const sid_engine* e, int i, sid_placement* out)
{
    if (!e || !out || i < 0 || i >= (int)e->devs.size()) return SID_EINVAL;
    const Dev& d = *e->devs[i];
    std::memset(out, 0, sizeof *out);
    out->device = d.device;
    out->gpu_numa_node = d.numa_node;
    out->cpus = d.ncpus;
    out->first_cpu = d.first_cpu;
    out->arena_numa_node = page_node(d.hh);
    out->ring_numa_node = d.pinned.empty() ? -1 : page_node(d.pinned[0]);
    std::memcpy(out->pci, d.pci, sizeof out->pci);
    out->pci[sizeof out->pci - 1] = 0;
    return SID_OK;
}

static void assign_devices(sid_engine* e)
{
    const int D = (int)e->devs.size();
    for (size_t j = 0; j < e->recs.size(); ++j) e->recs[j].dev = (int)(j % D);
}

// Pageable host text (a file's mapping, or host memory the caller did not
// pin) is uploaded chunk by chunk from registered pages: each chunk's page-
// aligned body is pinned (hipHostRegister, read-only) by the uploader while
// the previous chunk's DMA runs, copied straight from the page cache, and
// released once its copy is done; the partial pages at its ends (shared with
// the neighbouring chunks) take the runtime's pageable path.  Without it the
// runtime copies every byte through its own pinned staging buffers first
// (a CPU copy per byte: at a whole node's N uploads, host memory traffic).
// SID_UPLOAD_REGISTER=0: the pageable path for everything (A/B).
static bool upload_register()
{
    static const bool on = [] {
        const char* v = std::getenv("SID_UPLOAD_REGISTER");
        return !v || std::atoi(v) != 0;
    }();
    return on;
}

// host memory the runtime already maps for the device (pinned or registered)
static bool host_pinned(const char* p)
{
    hipPointerAttribute_t a;
    const bool pinned = hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeHost;
    (void)hipGetLastError();   // (pageable memory: an error to clear, not to report)
    return pinned;
}

extern "C" int sid_engine_source_text(sid_engine* e, const char* text, uint64_t len)
{
    if (!e || (!text && len)) return SID_EINVAL;
    drop_source(e);
    e->src = SRC_HOST;
    e->text = text;
    e->text_len = len;
    e->src_pinned = len && host_pinned(text);
    e->reg_upload = upload_register() && len && !e->src_pinned;
    split_host_text(e, text, len);
    assign_devices(e);
    return SID_OK;
}

extern "C" int sid_engine_source_file(sid_engine* e, int fd, uint64_t offset, uint64_t len)
{
    if (!e || fd < 0) return SID_EINVAL;
    struct stat sb;
    // a range past the end of the file would fault (SIGBUS) on the first read
    if (fstat(fd, &sb) != 0) return SID_EIO;
    if (S_ISREG(sb.st_mode) && (offset > (uint64_t)sb.st_size || len > (uint64_t)sb.st_size - offset))
        return SID_EINVAL;
    drop_source(e);
    if (len == 0) {
        e->src = SRC_HOST;
        return SID_OK;
    }
    const uint64_t pg = (uint64_t)sysconf(_SC_PAGESIZE);
    const uint64_t a = offset & ~(pg - 1);
    e->map_skew = offset - a;
    e->map_len = len + e->map_skew;
    // populated up front below 8 GiB (one kernel pass over the page tables was
    // measured fastest); larger inputs are populated chunk by chunk
    // ahead of the uploads and released behind them
    const bool populate = len <= (8ull << 30);
    void* m = mmap(nullptr, e->map_len, PROT_READ, MAP_PRIVATE | (populate ? MAP_POPULATE : 0), fd, (off_t)a);
    if (m == MAP_FAILED) return SID_EIO;
    (void)madvise(m, e->map_len, MADV_SEQUENTIAL);
    e->map = m;
    e->src = SRC_FILE;
    e->text = (const char*)m + e->map_skew;
    e->text_len = len;
    e->reg_upload = upload_register();
    split_host_text(e, e->text, len);
    assign_devices(e);
    return SID_OK;
}

// BGZF chunks: runs of whole members of at most chunk_bytes of text (at least
// one member), cut at line starts.  The cut in front of chunk j > 0 is one
// past the first '\n' at or after the text offset of its nominal first member
// (the line that straddles or starts at the boundary belongs to chunk j - 1;
// no newline before the end: the end), found by inflating that member alone
// on the host -- and the next ones while no newline appears.  A member that
// does not inflate counts as one without a newline: it then lies inside a
// chunk, whose device inflate reports it in file order.  Chunks whose cuts
// coincide (a line longer than a chunk) are dropped.
static void split_bgzf(sid_engine* e)
{
    const std::vector<sid_bgzf_blk>& B = e->zidx->blk;
    const uint8_t* z = (const uint8_t*)e->text;
    const uint64_t C = chunk_bytes(e), T = e->zidx->tlen;
    e->recs.clear();
    if (T == 0) return;
    std::vector<uint64_t> cuts{0};
    std::vector<uint8_t> buf(BGZF_MAX_ISIZE);
    for (size_t k = 0; k < B.size();) {
        uint64_t sum = 0;
        do sum += B[k++].isize;
        while (k < B.size() && sum + B[k].isize <= C);
        if (k == B.size()) break;
        uint64_t cut = T;
        if (cuts.back() > B[k].toff) {
            cut = cuts.back();   // the same newline: the previous cut's line runs past this member's start
        } else {
            for (size_t q = k; q < B.size(); ++q) {
                if (!B[q].isize) continue;
                if (sid_bgzf_inflate_block(z + B[q].coff, B[q].csize, B[q].isize, buf.data()) != BGZF_OK) continue;
                if (const void* nl = std::memchr(buf.data(), '\n', B[q].isize)) {
                    cut = B[q].toff + (uint64_t)((const uint8_t*)nl - buf.data()) + 1;
                    break;
                }
            }
        }
        cuts.push_back(cut);
    }
    cuts.push_back(T);
    // the member that holds text byte t (t < T)
    auto holds = [&](uint64_t t) {
        size_t lo = 0, hi = B.size();   // the last member with toff <= t: the empty ones in front of it share its toff
        while (hi - lo > 1) {
            const size_t mid = (lo + hi) / 2;
            if (B[mid].toff <= t) lo = mid;
            else hi = mid;
        }
        return lo;
    };
    for (size_t c = 0; c + 1 < cuts.size(); ++c) {
        const uint64_t a = cuts[c], b = cuts[c + 1];
        if (b <= a) continue;
        const size_t b0 = holds(a), b1 = holds(b - 1);
        ChunkRec r;
        r.toff = a;
        r.tlen = b - a;
        r.zb0 = b0;
        r.znb = b1 - b0 + 1;
        r.off = B[b0].coff;
        r.len = B[b1].coff + B[b1].csize - r.off;
        r.share = b < T && holds(b) == b1 ? B[b1].csize : 0;
        e->recs.push_back(r);
    }
}

extern "C" int sid_engine_source_bgzf(sid_engine* e, const void* bytes, uint64_t len, uint64_t* err_offset)
{
    if (err_offset) *err_offset = 0;
    if (!e || (!bytes && len)) return SID_EINVAL;
    drop_source(e);
    const int rc = sid_bgzf_index(bytes, len, &e->zidx, err_offset);
    if (rc != SID_OK) return rc;
    e->src = SRC_BGZF;
    e->text = (const char*)bytes;
    e->text_len = len;
    e->reg_upload = upload_register() && len && !host_pinned(e->text);
    split_bgzf(e);
    assign_devices(e);
    return SID_OK;
}

extern "C" int sid_engine_source_bgzf_file(sid_engine* e, int fd, uint64_t offset, uint64_t len, uint64_t* err_offset)
{
    if (err_offset) *err_offset = 0;
    int rc = sid_engine_source_file(e, fd, offset, len);   // the mapping; its text chunks are replaced below
    if (rc != SID_OK) return rc;
    e->recs.clear();
    rc = sid_bgzf_index(e->text, e->text_len, &e->zidx, err_offset);
    if (rc != SID_OK) {
        drop_source(e);
        return rc;
    }
    e->src = e->map ? SRC_BGZF_FILE : SRC_BGZF;
    split_bgzf(e);
    assign_devices(e);
    return SID_OK;
}

extern "C" int sid_engine_source_device_text(sid_engine* e, const char* d_text, uint64_t len)
{
    if (!e || (!d_text && len)) return SID_EINVAL;
    drop_source(e);
    e->src = SRC_DEVICE;
    e->text = d_text;
    e->text_len = len;
    // line-aligned cuts: a window around each nominal cut is read back
    Dev& d0 = *e->devs[0];
    if (hipSetDevice(d0.device) != hipSuccess) return SID_EHIP;
    const uint64_t C = chunk_bytes(e);
    std::vector<char> w(1 << 16);
    uint64_t at = 0;
    while (at < len) {
        uint64_t c = std::min(len, at + C);
        while (c < len) {   // the next '\n' at or after c - 1
            const uint64_t m = std::min<uint64_t>(w.size(), len - (c - 1));
            if (hipMemcpy(w.data(), d_text + c - 1, m, hipMemcpyDeviceToHost) != hipSuccess) return SID_EHIP;
            const char* nl = (const char*)std::memchr(w.data(), '\n', m);
            if (nl) {
                c = c - 1 + (uint64_t)(nl - w.data()) + 1;
                break;
            }
            c += m;
        }
        c = std::min(c, len);
        ChunkRec r;
        r.off = at;
        r.len = c - at;
        e->recs.push_back(r);
        at = c;
    }
    // the text lives on the first GPU: its pipelines take the chunks in turn
    const int lanes = std::max(1, e->cfg.lanes);
    for (size_t j = 0; j < e->recs.size(); ++j) e->recs[j].dev = (int)(j % std::min<size_t>(lanes, e->devs.size()));
    return SID_OK;
}

extern "C" int sid_engine_source_synth(sid_engine* e, uint64_t seed, double mean_depth, uint64_t first_site,
                                       uint64_t n, uint64_t sites_per_chrom, uint64_t sites_per_chunk, int on_device)
{
    if (!e || !(mean_depth >= 0) || mean_depth > 600) return SID_EINVAL;
    drop_source(e);
    e->src = on_device ? SRC_SYNTH_DEVICE : SRC_SYNTH_HOST;
    e->synth_seed = seed;
    e->synth_depth = mean_depth;
    e->synth_first = first_site;
    e->synth_n = n;
    e->synth_spc = sites_per_chrom;
    sid_poisson_cdf(mean_depth, e->synth_cdf);
    // about 2.7 B per read (base, quality, marks) + 20 B of fields per site
    const double per_site = 20.0 + 2.75 * mean_depth;
    uint64_t per = sites_per_chunk ? sites_per_chunk : (uint64_t)(chunk_bytes(e) / per_site);
    per = std::max<uint64_t>(per, 1);
    e->synth_per = per;
    // capacity: the mean plus a wide margin (the generator reports overflow)
    e->per_chunk_cap = (uint64_t)(per * per_site * 1.25) + (64ull + 5ull * e->synth_cdf.size()) + (1u << 20);
    for (uint64_t s = 0; s < n; s += per) {
        ChunkRec r;
        r.site0 = first_site + s;
        r.nsites = std::min(per, n - s);
        e->recs.push_back(r);
    }
    assign_devices(e);
    if (on_device) {
        const size_t D = e->devs.size();
        e->d_cdf_dev.resize(D, nullptr);
        e->gen_ws.resize(D);
        for (size_t i = 0; i < D; ++i) {
            if (hipSetDevice(e->devs[i]->device) != hipSuccess) return SID_EHIP;
            if (e->d_cdf_dev[i]) (void)hipFree(e->d_cdf_dev[i]);
            e->d_cdf_dev[i] = nullptr;
            if (hipMalloc(&e->d_cdf_dev[i], e->synth_cdf.size() * 8) != hipSuccess ||
                hipMemcpy(e->d_cdf_dev[i], e->synth_cdf.data(), e->synth_cdf.size() * 8, hipMemcpyHostToDevice) !=
                    hipSuccess)
                return SID_EHIP;
        }
    }
    return SID_OK;
}

// --------------------------------------------------------------- threads --
namespace {

bool needs_format_pass1(const sid_engine* e) { return !e->lynch; }

// The device sink (cfg.device_sink 1: records formatted into HBM and dropped)
// formats every -m local / quality chunk in pass 1 into a pooled scratch
// buffer whose bytes are counted and dropped at once (no hold arena, whose
// HBM a 2 GiB chunk's record bound then lacked beside C4's 244 GB of
// resident text: SID_ENOMEM, profiles/bench_c4_2gib_chunks_r04.err).  Nothing is written
// anywhere, so the all-or-nothing output that makes the other sinks hold
// records until every chunk is validated does not apply, and no chunk is
// indexed and parsed a second time in pass 2 (C4 on one GPU: 131 GB of
// records against a hold budget of ~16 GB).
bool sink_all_pass1(const sid_engine* e) { return e->cfg.device_sink == 1 && needs_format_pass1(e); }

// An uploader's registered chunk bodies (upload_register): at most the one
// being copied and the next, each released once its copy's event is done.
struct UploadReg {
    struct Reg {
        uint64_t j = UINT64_MAX;
        char* p = nullptr;          // page-aligned body, registered
        uint64_t n = 0;
        hipEvent_t ev = nullptr;    // its copy done
        bool copied = false;
    };
    sid_engine* e;
    bool on;
    std::deque<Reg> regs;
    std::vector<hipEvent_t> evs;
    UploadReg(sid_engine* e_, int pass) : e(e_), on(e_->reg_upload && (pass == 1 || src_file(e_->src))) {}
    ~UploadReg()
    {
        for (auto& r : regs) {
            if (r.ev) (void)hipEventSynchronize(r.ev);
            unregister(r.p);
        }
        for (auto& r : regs)
            if (r.ev) (void)hipEventDestroy(r.ev);
        for (hipEvent_t ev : evs) (void)hipEventDestroy(ev);
    }
    Reg* find(uint64_t j)
    {
        for (auto& r : regs)
            if (r.j == j) return &r;
        return nullptr;
    }
    // pin chunk j's whole pages (bodies of at least 1 MiB; smaller chunks
    // take the pageable path, and so does every chunk after a registration
    // fails)
    void pin(uint64_t j)
    {
        if (!on || j == UINT64_MAX || find(j)) return;
        const ChunkRec& r = e->recs[j];
        const uint64_t pg = (uint64_t)sysconf(_SC_PAGESIZE);
        const uintptr_t s = (uintptr_t)(e->text + r.off), t = s + r.len - r.share;   // (pages are registered once)
        const uintptr_t a = (s + pg - 1) & ~(uintptr_t)(pg - 1), b = t & ~(uintptr_t)(pg - 1);
        if (b <= a || b - a < (1u << 20)) return;
        const double t0 = wall();
        const bool ok = hipHostRegister((void*)a, b - a, hipHostRegisterReadOnly) == hipSuccess ||
                        ((void)hipGetLastError(), hipHostRegister((void*)a, b - a, hipHostRegisterDefault) == hipSuccess);
        e->t_register += (uint64_t)((wall() - t0) * 1e9);
        if (!ok) {
            (void)hipGetLastError();   // not an error: the pageable path from now on
            on = false;
            return;
        }
        Reg g;
        g.j = j;
        g.p = (char*)a;
        g.n = b - a;
        regs.push_back(g);
    }
    void ahead(uint64_t j)
    {
        release_done();
        pin(j);
    }
    // chunk j (pinned now if it is not yet) into dst on stream st
    hipError_t copy(char* dst, uint64_t j, hipStream_t st)
    {
        const ChunkRec& r = e->recs[j];
        const char* src = e->text + r.off;
        pin(j);
        Reg* g = find(j);
        if (!g) return hipMemcpyAsync(dst, src, r.len, hipMemcpyHostToDevice, st);
        const uint64_t head = (uint64_t)(g->p - src), body = g->n, tail = r.len - head - body;
        hipError_t x = hipSuccess;
        if (head) x = hipMemcpyAsync(dst, src, head, hipMemcpyHostToDevice, st);
        if (x == hipSuccess) x = hipMemcpyAsync(dst + head, g->p, body, hipMemcpyHostToDevice, st);
        if (x == hipSuccess) e->reg_chunks++;
        if (x == hipSuccess && tail) x = hipMemcpyAsync(dst + head + body, g->p + body, tail, hipMemcpyHostToDevice, st);
        if (x == hipSuccess) {
            if (evs.empty()) {
                hipEvent_t ev = nullptr;
                x = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
                if (x == hipSuccess) evs.push_back(ev);
            }
            if (x == hipSuccess) {
                g->ev = evs.back();
                evs.pop_back();
                x = hipEventRecord(g->ev, st);
                g->copied = true;
            }
        }
        return x;
    }
    void unregister(char* p)
    {
        const double t0 = wall();
        (void)hipHostUnregister(p);
        e->t_register += (uint64_t)((wall() - t0) * 1e9);
    }
    // unregister the bodies whose copies are done (in copy order)
    void release_done()
    {
        while (!regs.empty() && regs.front().copied && hipEventQuery(regs.front().ev) == hipSuccess) {
            unregister(regs.front().p);
            evs.push_back(regs.front().ev);
            regs.pop_front();
        }
        (void)hipGetLastError();   // (hipEventQuery's "not ready")
    }
};

// The uploads of this run may be stripped (sid_engine_cfg.strip): host text that is pinned already, and
// an option set that reads nothing behind a line's read bases (-m quality reads both quality columns)
bool strip_eligible(const sid_engine* e)
{
    return e->strip_T >= 2 && e->src == SRC_HOST && e->src_pinned && !e->reg_upload &&
           e->opts.method != SID_METHOD_QUALITY;
}

// thread t of device d's strip crew (StripRun): its region of every job, in the uploader's order
void strip_worker(sid_engine* e, Dev& d, StripRun& S, const std::vector<uint64_t>& list, int t)
{
    bind_thread(d);
    if (t == 0) (void)hipSetDevice(d.device);   // (the leader waits for the staging buffers' events)
    double busy = 0;
    for (uint64_t k = 0; k < S.jobs.size(); ++k) {
        if (!S.wanted(k)) continue;
        const int b = (int)(k % Dev::STRIP_RING);
        {
            std::unique_lock<std::mutex> l(S.m);
            if (t == 0) {
                // the buffer's last job: taken by the uploader, and left by every thread -- one that was
                // taken goes on writing into its region until its next tick
                uint64_t last = k;
                while (last >= (uint64_t)Dev::STRIP_RING && !S.wanted(last -= Dev::STRIP_RING)) {
                }
                if (last != k && S.wanted(last))
                    S.cv.wait(l, [&] { return S.stop || (S.decided > last && S.fin[last] == S.T); });
                if (S.stop) break;
                if (S.sev_used[b]) {
                    l.unlock();
                    (void)hipEventSynchronize(d.sev[b]);
                    l.lock();
                }
                S.ready = k + 1;
                S.cv.notify_all();
            } else {
                S.cv.wait(l, [&] { return S.stop || S.ready > k; });
            }
            if (S.stop) break;
        }
        StripJob& J = S.jobs[k];
        StripProg& P = J.P[t];
        bool go;
        {
            std::lock_guard<std::mutex> l(P.m);
            go = !P.taken;
        }
        if (go) {
            const double t0 = wall();
            (void)sid_strip_stream(e->text + e->recs[list[k]].off + J.cut[t], J.cut[t + 1] - J.cut[t],
                                   d.sbuf[b] + S.place(J, t), STRIP_STEP,
                                   [](void* u, uint64_t in_done, uint64_t out_done, uint64_t lines) {
                                       StripProg& Q = *(StripProg*)u;
                                       std::lock_guard<std::mutex> l(Q.m);
                                       if (Q.taken) return false;
                                       Q.in_done = in_done, Q.out_done = out_done, Q.lines = lines;
                                       return true;
                                   },
                                   &P);
            busy += wall() - t0;
        }
        std::lock_guard<std::mutex> l(S.m);
        if (++S.fin[k] == S.T) S.cv.notify_all();
    }
    const uint64_t ns = (uint64_t)(busy * 1e9);
    e->t_strip += ns;
    for (uint64_t c = e->t_strip_min.load(); ns < c && !e->t_strip_min.compare_exchange_weak(c, ns);) {
    }
    for (uint64_t c = e->t_strip_max.load(); ns > c && !e->t_strip_max.compare_exchange_weak(c, ns);) {
    }
}

// the uploader of device d: the chunks of `list` into device buffers, in order
// (S: the device's strip crew in this pass, or null)
void uploader(sid_engine* e, Dev& d, const std::vector<uint64_t>& list, int pass, StripRun* S = nullptr)
{
    bind_thread(d);
    // (however this thread leaves: the crew stops waiting for it)
    struct CrewStop {
        StripRun* S;
        ~CrewStop()
        {
            if (!S) return;
            std::lock_guard<std::mutex> l(S->m);
            S->stop = true;
            S->cv.notify_all();
        }
    } crew_stop{S};
    if (hipSetDevice(d.device) != hipSuccess) return (void)fail(e, SID_EHIP);
    UploadReg reg(e, pass);
    // the ingest's uploads timed as one span on the upload stream, from the
    // first copy's start to the last one's end (the copies run back to back;
    // a pair of events around every copy cost the step ~0.3 ms)
    struct Span {
        Dev& d;
        hipEvent_t t0 = nullptr;
        uint64_t bytes = 0;
        ~Span()
        {
            if (!t0) return;
            hipEvent_t t1 = d.h2d_event();
            if (t1 && hipEventRecord(t1, d.s_up) == hipSuccess) {
                d.h2d_pending.push_back({t0, t1});
                d.h2d_bytes += bytes;
            } else {
                d.h2d_free.push_back(t0);
                if (t1) d.h2d_free.push_back(t1);
            }
        }
    } span{d};
    // the chunk this uploader copies after j from the host (UINT64_MAX: none)
    size_t at = 0;
    auto next_of = [&](uint64_t j) -> uint64_t {
        while (at < list.size() && list[at] != j) ++at;
        for (size_t k = at + 1; k < list.size(); ++k) {
            const ChunkRec& q = e->recs[list[k]];
            if (pass == 2 && (q.host1 || q.sunk || q.held || q.kept)) continue;
            return list[k];
        }
        return UINT64_MAX;
    };
    // Chunk j = job k of the crew, into dst: every region as far as its thread got -- those bytes from
    // the staging buffer, the region's rest from the source (neighbouring rests in one copy).  Without
    // cfg.strip 1 / 2 the link does not wait for the crew: the chunk is taken once the crew has left it,
    // or the copies before it on the stream are done (prev_up), whichever comes first.
    hipEvent_t prev_up = nullptr;   // the chunk before's upload done (null: it was waited for)
    auto strip_copy = [&](uint64_t k, ChunkRec& r, char* dst, Loaded& L, uint64_t* moved) -> hipError_t {
        StripJob& J = S->jobs[k];
        const int T = S->T, b = (int)(k % Dev::STRIP_RING);
        const char* src = e->text + r.off;
        if (S->wanted(k)) {
            std::unique_lock<std::mutex> l(S->m);
            while (S->fin[k] < T && e->rc.load() == SID_OK) {
                if (S->mode == 0) {
                    l.unlock();
                    const bool idle = !prev_up || hipEventQuery(prev_up) == hipSuccess;
                    (void)hipGetLastError();   // (hipErrorNotReady)
                    l.lock();
                    if (idle) break;
                }
                S->cv.wait_for(l, std::chrono::microseconds(S->mode == 0 ? 50 : 1000));
            }
        }
        hipError_t x = hipSuccess;
        uint64_t o = 0, raw0 = 0, rawn = 0;   // the device offset; the source bytes waiting for their copy
        bool staged = false;
        r.smap.clear();
        auto flush_raw = [&] {
            if (!rawn) return;
            if (x == hipSuccess) x = hipMemcpyAsync(dst + o, src + raw0, rawn, hipMemcpyHostToDevice, d.s_up);
            r.smap.push_back({rawn, rawn, false});
            o += rawn;
            rawn = 0;
        };
        for (int t = 0; t < T; ++t) {
            uint64_t in_done, out_done, lines;
            {
                std::lock_guard<std::mutex> l(J.P[t].m);
                J.P[t].taken = true;
                in_done = J.P[t].in_done, out_done = J.P[t].out_done, lines = J.P[t].lines;
            }
            const uint64_t a = J.cut[t], n = J.cut[t + 1] - a;
            if (in_done) {
                flush_raw();
                if (x == hipSuccess)
                    x = hipMemcpyAsync(dst + o, d.sbuf[b] + S->place(J, t), out_done, hipMemcpyHostToDevice, d.s_up);
                r.smap.push_back({out_done, in_done, true});
                o += out_done;
                staged = true;
                L.lines += lines;
                L.lbytes += out_done;
            }
            if (in_done < n) {
                if (!rawn) raw0 = a + in_done;
                rawn += n - in_done;
            }
        }
        flush_raw();
        if (staged && x == hipSuccess) x = hipEventRecord(d.sev[b], d.s_up);
        {
            std::lock_guard<std::mutex> l(S->m);
            S->sev_used[b] |= staged;
            S->decided = k + 1;
            S->cv.notify_all();
        }
        if (o < r.len) {
            e->strip_chunks++;
            e->strip_bytes += r.len - o;
        } else {
            r.smap.clear();   // (nothing dropped: the bytes are the input's)
        }
        *moved = o;
        return x;
    };
    // Pass 2 reads a chunk again whose upload in pass 1 was stripped: the same bytes again, piece by piece
    // (ChunkRec::smap; a piece's stripped form depends on its bytes alone) -- the parse kept since pass 1
    // (ChunkRec::pre) holds line offsets into them.  Stripped by this thread into the first staging
    // buffer, which no crew uses in pass 2, and waited for.
    auto strip_again = [&](ChunkRec& r, char* dst, uint64_t* moved) -> hipError_t {
        const char* src = e->text + r.off;
        hipError_t x = hipSuccess;
        uint64_t o = 0, raw = 0, so = 0;
        for (const auto& g : r.smap) {
            if (x != hipSuccess) break;
            if (!g.stripped) {
                x = hipMemcpyAsync(dst + o, src + raw, g.raw, hipMemcpyHostToDevice, d.s_up);
            } else {
                if (so + g.raw > d.scap) {   // (the buffer's earlier pieces copied first)
                    x = hipStreamSynchronize(d.s_up);
                    so = 0;
                }
                if (x != hipSuccess || g.raw > d.scap) return x != hipSuccess ? x : hipErrorUnknown;
                const size_t m = sid_strip_lines(src + raw, g.raw, d.sbuf[0] + so, g.raw, nullptr);
                if (m != g.dev) return hipErrorUnknown;   // cannot happen: the bytes pass 1 stripped
                x = hipMemcpyAsync(dst + o, d.sbuf[0] + so, m, hipMemcpyHostToDevice, d.s_up);
                so += (m + 63) & ~(uint64_t)63;
            }
            o += g.dev;
            raw += g.raw;
        }
        if (x == hipSuccess) x = hipStreamSynchronize(d.s_up);
        *moved = o;
        return x;
    };
    uint64_t jobs = 0;
    for (uint64_t j : list) {
        const uint64_t k = jobs++;   // (pass 1 of host text: every chunk of the list gets here, the crew's job k)
        if (e->rc.load() != SID_OK) break;
        if (pass == 1 && j > e->first_err.load()) break;
        ChunkRec& r = e->recs[j];
        Loaded L;
        L.j = j;
        if (pass == 2 && (r.host1 || r.sunk)) continue;   // in host memory already (the writer takes it), or sunk
        if (pass == 2 && r.held) {
            L.kind = 1;
            if (!d.loaded.push(L)) break;
            continue;
        }
        if (e->src == SRC_DEVICE) {   // resident text: a view, 16-B aligned base
            const uint64_t a = (uint64_t)(uintptr_t)(e->text + r.off);
            L.base = (const char*)(uintptr_t)(a & ~(uint64_t)15);
            L.c0 = a & 15;
            L.c1 = L.c0 + r.len;
            if (!d.loaded.push(L)) break;
            continue;
        }
        if (pass == 2 && r.kept) {
            L.base = r.kept + r.kept_head;
            L.c0 = 0;
            L.c1 = r.kept_len;
            if (!d.loaded.push(L)) break;
            continue;
        }
        // text length (synthetic sources: a bound until generated)
        const bool bgzf = src_bgzf(e->src);
        uint64_t need = e->src == SRC_SYNTH_HOST || e->src == SRC_SYNTH_DEVICE ? e->per_chunk_cap
                        : bgzf                                                   ? r.tlen + 2 * ZHEAD
                                                                                 : r.len;
        // keep it for pass 2?  Lynch always needs a second pass; local and
        // quality only once the hold budget ran out
        // (the device sink formats every -m local / quality chunk in pass 1:
        // nothing to keep for a second pass)
        bool want_keep = pass == 1 && (e->lynch || (d.hold_full.load() && !sink_all_pass1(e))) &&
                         d.retain_used.load() + need + PAD <= d.retain_budget;
        char* dst = nullptr;
        uint64_t dcap = 0;
        int slot = -1;
        hipError_t x = hipSuccess;
        if (want_keep) {
            dst = d.pool.get(need + PAD, &dcap, d.s_up);
            if (dst) d.retain_used += dcap;
            else want_keep = false;   // no HBM for it: a ring slot, read again in pass 2
        }
        if (!want_keep) {
            if (!d.free_slots.pop(slot)) break;
            Slot& s = d.slots[slot];
            if (s.cap < need) {   // grow: wait for the slot's last reader first
                if (s.used) x = hipEventSynchronize(s.ev_free);
                if (s.text) (void)hipFree(s.text);
                s.text = nullptr;
                s.cap = 0;
                const uint64_t c = std::max<uint64_t>(need, chunk_bytes(e) + (chunk_bytes(e) >> 3));
                if (x == hipSuccess) x = hipMalloc(&s.text, c + PAD);
                if (x == hipSuccess) s.cap = c;
                s.used = false;
            } else if (s.used) {
                // the slot's last reader (compute stream) is long done by now:
                // waited for here, not by the copy engine's queue (a cross-
                // queue wait in front of every copy)
                x = hipEventSynchronize(s.ev_free);
            }
            if (x != hipSuccess) return (void)hipfail(e, x);
            dst = s.text;
            dcap = s.cap + PAD;
            s.used = true;
        }
        uint64_t len = r.len;
        // BGZF: the compressed bytes go to the device's staging buffer, the member table behind them
        char* cdst = dst;
        sid_bgzf_dblk* d_ztab = nullptr;
        uint64_t zn = 0, zbad_empty = ~0ull;   // the members that hold text; the first bad empty one's offset
        if (bgzf) {
            const uint64_t zb = (r.len + 15) & ~(uint64_t)15, tb = r.znb * sizeof(sid_bgzf_dblk);
            const uint64_t all = zb + tb + r.znb * 4 + 16;
            if (d.zcap < all) {   // (the stream is idle: every BGZF chunk ends in a sync)
                if (d.zbuf) (void)hipFree(d.zbuf);
                d.zbuf = nullptr;
                d.zcap = 0;
                x = hipMalloc(&d.zbuf, all + (all >> 2));
                if (x == hipSuccess) d.zcap = all + (all >> 2);
            }
            if (x == hipSuccess && d.ztab_cap < 16 + tb) {
                if (d.ztab_h) (void)hipHostFree(d.ztab_h);
                d.ztab_h = nullptr;
                d.ztab_cap = 0;
                x = hipHostMalloc((void**)&d.ztab_h, 16 + tb + (tb >> 2), hipHostMallocDefault);
                if (x == hipSuccess) d.ztab_cap = 16 + tb + (tb >> 2);
            }
            if (x != hipSuccess) return (void)hipfail(e, x);
            // (the kernel takes the members that hold text; an empty one is checked here, by the host build
            // of the same decoder, and the lowest bad member of either kind is the chunk's)
            sid_bgzf_dblk* h = (sid_bgzf_dblk*)(d.ztab_h + 16);
            zn = 0;
            zbad_empty = ~0ull;
            for (uint64_t k = 0; k < r.znb; ++k) {
                const sid_bgzf_blk& b = e->zidx->blk[r.zb0 + k];
                uint8_t none;
                if (b.isize) h[zn++] = sid_bgzf_dblk{b.coff - r.off, (int64_t)b.toff - (int64_t)r.toff, b.csize, b.isize};
                else if (zbad_empty == ~0ull &&
                         sid_bgzf_inflate_block((const uint8_t*)e->text + b.coff, b.csize, 0, &none) != BGZF_OK)
                    zbad_empty = b.coff;
            }
            cdst = d.zbuf;
            d_ztab = (sid_bgzf_dblk*)(d.zbuf + zb);
            dst += ZHEAD;   // the chunk's first line
            dcap -= ZHEAD;
        }
        if (src_host(e->src) || src_file(e->src)) {
            if (pass == 1 && len && !span.t0 && (span.t0 = d.h2d_event())) x = hipEventRecord(span.t0, d.s_up);
            if (len && x == hipSuccess) x = S                                ? strip_copy(k, r, cdst, L, &len)
                                            : pass == 2 && !r.smap.empty() ? strip_again(r, cdst, &len)
                                                                           : reg.copy(cdst, j, d.s_up);
            if (pass == 1 && span.t0 && x == hipSuccess) span.bytes += len;
            // the next chunk's pages pinned while this copy runs; the ones
            // whose copies are done released
            if (x == hipSuccess) reg.ahead(next_of(j));
            if (src_file(e->src) && x == hipSuccess && e->text_len > (8ull << 30)) {
                // large mapped inputs: drop the chunk's page-table entries once
                // copied (the page cache keeps the data; RSS stays bounded)
                x = hipStreamSynchronize(d.s_up);
                reg.release_done();
                const uint64_t pg = (uint64_t)sysconf(_SC_PAGESIZE);
                const uint64_t a = (e->map_skew + r.off + pg - 1) & ~(pg - 1);
                const uint64_t b = (e->map_skew + r.off + len) & ~(pg - 1);
                if (b > a) (void)madvise((char*)e->map + a, b - a, MADV_DONTNEED);
            }
            if (bgzf && x == hipSuccess) {
                // inflated on the upload stream into the text buffer, and waited for: a bad member is
                // known before the chunk reaches the compute stage
                uint32_t* d_status = (uint32_t*)(d_ztab + zn);
                uint32_t* bad = (uint32_t*)d.ztab_h;
                *bad = 0xffffffffu;
                if (zn) x = hipMemcpyAsync(d_ztab, d.ztab_h + 16, zn * sizeof(sid_bgzf_dblk), hipMemcpyHostToDevice, d.s_up);
                if (x == hipSuccess)
                    x = sid_launch_bgzf_inflate((const uint8_t*)d.zbuf, d_ztab, (uint32_t)zn, (uint8_t*)dst, d_status,
                                                d_status + zn, d.s_up);
                if (x == hipSuccess) x = hipMemcpyAsync(bad, d_status + zn, 4, hipMemcpyDeviceToHost, d.s_up);
                if (x == hipSuccess) x = hipStreamSynchronize(d.s_up);
                if (x != hipSuccess) return (void)hipfail(e, x);
                if (pass == 1) e->z_bytes += r.len - r.share, e->z_blocks += r.znb - (r.share != 0);   // (each member once)
                len = r.tlen;
                if (*bad != 0xffffffffu || zbad_empty != ~0ull) {
                    if (pass == 2) return (void)fail(e, SID_EBGZF);   // cannot happen: pass 1 inflated the same bytes
                    const sid_bgzf_dblk* h = (const sid_bgzf_dblk*)(d.ztab_h + 16);
                    r.zbad = std::min<uint64_t>(zbad_empty, *bad != 0xffffffffu ? r.off + h[*bad].coff : UINT64_MAX);
                    uint64_t cur = e->first_err.load();
                    while (j < cur && !e->first_err.compare_exchange_weak(cur, j)) {
                    }
                    if (slot >= 0) {
                        (void)hipEventRecord(d.slots[slot].ev_free, d.s_up);
                        d.free_slots.push(slot);
                    } else {
                        d.pool.put(dst - ZHEAD, dcap + ZHEAD, d.s_up);
                        d.retain_used -= dcap + ZHEAD;
                    }
                    continue;
                }
            }
        } else if (e->src == SRC_SYNTH_HOST) {
            // generated by host threads into this device's pinned staging,
            // one region per thread, each region DMA'd to its place
            const size_t gi = (size_t)d.index;
            const int T = std::max(1, e->cfg.host_threads > 0 ? e->cfg.host_threads : 8);
            const uint64_t region = e->per_chunk_cap / T + e->per_chunk_cap / (4 * T) + 64 + 5 * e->synth_cdf.size();
            x = hipEventSynchronize(e->gen_ev[gi]);   // the previous chunk's copies are done
            if (x == hipSuccess && e->gen_cap[gi] < region * T) {
                if (e->gen_buf[gi]) (void)hipHostFree(e->gen_buf[gi]);
                e->gen_buf[gi] = nullptr;
                e->gen_cap[gi] = 0;
                x = hipHostMalloc((void**)&e->gen_buf[gi], region * T, hipHostMallocDefault);
                if (x == hipSuccess) e->gen_cap[gi] = region * T;
            }
            std::vector<uint64_t> plen(T, 0);
            if (x == hipSuccess) {
                std::vector<std::thread> th;
                for (int t = 0; t < T; ++t)
                    th.emplace_back([&, t] {
                        const uint64_t a = r.nsites * t / T, b = r.nsites * (t + 1) / T;
                        plen[t] = synth_host(e->synth_cdf, e->synth_seed, r.site0 + a, b - a, e->synth_spc,
                                             e->gen_buf[gi] + region * t, region);
                    });
                for (auto& t : th) t.join();
            }
            len = 0;
            for (int t = 0; t < T && x == hipSuccess; ++t) {
                if (plen[t] == UINT64_MAX || len + plen[t] > dcap - PAD) return (void)fail(e, SID_ENOMEM);
                if (plen[t])
                    x = hipMemcpyAsync(dst + len, e->gen_buf[gi] + region * t, plen[t], hipMemcpyHostToDevice,
                                       d.s_up);
                len += plen[t];
            }
            if (x == hipSuccess) x = hipEventRecord(e->gen_ev[gi], d.s_up);
        } else if (e->src == SRC_SYNTH_DEVICE) {
            sid_synth_gen_ws& G = e->gen_ws[d.index];
            x = sid_launch_synth_text(e->synth_seed, e->d_cdf_dev[d.index], (uint32_t)e->synth_cdf.size(), r.site0,
                                      r.nsites, e->synth_spc, &G, dst, dcap - PAD, d.s_up, e->synth_depth);
            if (x == hipSuccess) x = hipMemcpyAsync(d.h_small + 6, G.res, 16, hipMemcpyDeviceToHost, d.s_up);
            if (x == hipSuccess) x = hipStreamSynchronize(d.s_up);
            if (x == hipSuccess) {
                if (d.h_small[7]) return (void)fail(e, SID_ENOMEM);   // beyond the generator's margin
                len = d.h_small[6];
            }
        }
        // the bytes past the chunk only need to be readable (every kernel
        // bounds its reads by the chunk's end), which the buffers' PAD
        // guarantees; zeroing them per chunk put a fill kernel between every
        // two copies of the upload stream (copy engine -> shader -> copy
        // engine), so it is done only where a kernel already wrote the text
        if (x == hipSuccess && e->src == SRC_SYNTH_DEVICE) x = hipMemsetAsync(dst + len, 0, PAD, d.s_up);
        hipEvent_t ev = nullptr;
        if (slot >= 0) {
            ev = d.slots[slot].ev_up;
            if (x == hipSuccess) x = hipEventRecord(ev, d.s_up);
        } else if (x == hipSuccess) {
            x = hipStreamSynchronize(d.s_up);   // kept buffers: no per-buffer event
        }
        if (x != hipSuccess) return (void)hipfail(e, x);
        if (want_keep) {
            r.kept_head = bgzf ? ZHEAD : 0;
            r.kept = dst - r.kept_head;
            r.kept_cap = dcap + r.kept_head;
            r.kept_len = len;
        }
        L.slot = slot;
        L.base = dst;
        L.c0 = 0;
        L.c1 = len;
        L.ev = ev;
        prev_up = ev;
        if (pass == 2) e->reloaded++;
        if (!d.loaded.push(L)) break;
    }
    d.loaded.close();
}

int call_sites(sid_engine* e, Dev& d, const Loaded& L, uint64_t n)
{
    sid_chunk_ws& W = d.ws;
    if (n == 0) return SID_OK;
    const int m = e->opts.method;
    if (m == SID_METHOD_QUALITY) return sid_chunk_quality(d.ctx, &W, L.base, L.c1, n, d.s_comp);
    if (m == SID_METHOD_LOCAL)
        return sid_call_local(d.ctx, (const uint16_t*)W.counts, n, W.code, W.hom, W.het, d.s_comp);
    return sid_lookup_sites(d.ctx, (const uint16_t*)W.counts, n, W.code, W.hom, W.het, d.s_comp);
}

// The sets (sid_chunk_ws::win_cur, dh.cur, rs.cur) a chunk's stages wrote, -1 before any ran: the next chunk's
// tile parse takes the other ones before this chunk's rows are read
struct StageSets {
    int win = -1, dh = -1, rs = -1;
};
static StageSets stage_sets(const sid_chunk_ws& W) { return StageSets{W.win_cur, W.dh.cur, W.rs.cur}; }

// A chunk's rows out of set b of a bin table (the depth histogram's, the region rows'): the set's pinned block,
// which holds `eager` rows behind its count, or beyond them a copy of their own and sync().  limit: the table's
// bins -- a set holds them all, so no chunk runs again for it
template <class Bin, class Row, class Sync>
static hipError_t bins_take(const sid_bin_sets<Bin, Row>& T, int b, uint64_t limit, uint32_t eager, std::vector<Row>& c,
                            hipStream_t st, Sync&& sync)
{
    const char* hb = T.eager[b];
    const uint64_t nr = *(const uint64_t*)hb;
    if (nr > limit) return hipErrorUnknown;
    c.resize(nr);
    if (nr <= eager) {
        if (nr) std::memcpy(c.data(), hb + 16, nr * sizeof(Row));
        return hipSuccess;
    }
    hipError_t x = hipMemcpyAsync(c.data(), T.rows[b], nr * sizeof(Row), hipMemcpyDeviceToHost, st);
    if (x == hipSuccess) x = sync();
    return x;
}

// the compute thread of device d, for one pass
void compute(sid_engine* e, Dev& d, int pass)
{
    bind_thread(d);
    if (hipSetDevice(d.device) != hipSuccess) return (void)fail(e, SID_EHIP);
    sid_chunk_ws& W = d.ws;
    uint64_t* hs = d.h_small;
    const int qmode = e->quality ? 1 : 0;
    auto sync = [&]() {
        const double a = wall();
        const hipError_t r = hipStreamSynchronize(d.s_comp);
        e->t_comp_sync += (uint64_t)((wall() - a) * 1e9);
        return r;
    };
    // (an event instead of the stream: the work queued behind it is not waited for)
    auto sync_ev = [&](hipEvent_t ev) {
        const double a = wall();
        const hipError_t r = hipEventSynchronize(ev);
        e->t_comp_sync += (uint64_t)((wall() - a) * 1e9);
        return r;
    };
    // the next chunk, taken early so that its line index runs behind this
    // chunk's formatter (the GPU then does not idle over the host round trip
    // that reads the formatter's byte count); indexed: its site count is in hs[0]
    Loaded nextL;
    bool have_next = false, next_indexed = false;
    // ... or its tile parse behind this chunk's writer (tiled: with next_lg
    // slots a tile, the next_quad shape)
    bool next_tiled = false, next_quad = false;
    uint32_t next_lg = 0;
    // ... and the sets its stages wrote
    StageSets next_sets;
    // the windowed summary
    const bool windows = e->opts.window > 0;
    // (the stage's last kernel stores its counts and first rows into the set's pinned block: win_eager)
    // after the sync: the set held every row and name of the chunk
    auto win_fits = [&](int b) {
        const uint64_t* hw = (const uint64_t*)W.win_eager[b];
        return hw[0] <= W.win_cap[b] && hw[1] <= W.win_ncap[b];
    };
    // ... and the sizes the next chunks' sets get (the tile path has no round trip to size them in)
    auto win_want = [&](int b) {
        const uint64_t* hw = (const uint64_t*)W.win_eager[b];
        W.win_want_rows = std::max<uint64_t>(W.win_want_rows, hw[0] + hw[0] / 2);
        W.win_want_names = std::max<uint64_t>(W.win_want_names, hw[1] + hw[1] / 2);
    };
    // the chunk's rows into its record: the pinned copy, or (more rows than it holds) a copy of their own
    auto win_take = [&](int b, sid_win_chunk& c) {
        const char* hb = W.win_eager[b];
        const uint64_t* hw = (const uint64_t*)hb;
        const uint64_t nr = hw[0], nn = hw[1];
        c.rows.resize(nr);
        c.names.resize(nn);
        if (nr <= SID_WIN_EAGER_ROWS && nn <= SID_WIN_EAGER_NAMES) {
            if (nr) std::memcpy(c.rows.data(), hb + WIN_H_ROWS, nr * sizeof(sid_win_row));
            if (nn) std::memcpy(&c.names[0], hb + WIN_H_NAMES, nn);
            return hipSuccess;
        }
        hipError_t x = hipSuccess;
        if (nr) x = hipMemcpyAsync(c.rows.data(), W.win_rows[b], nr * sizeof(sid_win_row), hipMemcpyDeviceToHost, d.s_comp);
        if (x == hipSuccess && nn) x = hipMemcpyAsync(&c.names[0], W.win_names[b], nn, hipMemcpyDeviceToHost, d.s_comp);
        if (x == hipSuccess) x = sync();
        return x;
    };
    // the depth histogram and the region rows (bins_take)
    const bool dhist = e->depth_hist;
    const bool rstats = e->region_stats;
    auto take = [&](Loaded& out) {
        if (have_next) {
            out = nextL;
            have_next = false;
            return true;
        }
        return d.loaded.pop(out);
    };
    Loaded L;
    while (take(L)) {
        const bool pre_indexed = next_indexed;
        next_indexed = false;
        bool pre_tiled = next_tiled;
        next_tiled = false;
        if (e->rc.load() != SID_OK) break;
        ChunkRec& r = e->recs[L.j];
        auto release_slot = [&]() {
            if (L.slot < 0) return;
            (void)hipEventRecord(d.slots[L.slot].ev_free, d.s_comp);
            d.free_slots.push(L.slot);
        };
        if (L.kind == 1) {   // pass 2: records held since pass 1
            OutItem it;
            it.j = L.j;
            it.buf = r.held;
            it.cap = r.held_cap;
            it.len = r.held_len;
            r.held = nullptr;
            if (e->cfg.device_sink == 1) e->sink_bytes += it.len, d.pool.put(it.buf, it.cap, nullptr);
            else if (!d.drain_q.push(it)) break;
            continue;
        }
        if (pass == 1 && L.j > e->first_err.load()) {
            if (pre_tiled) W.slot_cap = 0;
            release_slot();
            continue;
        }
        int rc = SID_OK;
        hipError_t x = hipSuccess;
        if (L.ev && !pre_indexed && !pre_tiled) x = hipStreamWaitEvent(d.s_comp, L.ev, 0);
        if (!pre_tiled) d.tile_ahead(L.lines, L.lbytes);   // (stripped text: slots for its lines per byte)
        const bool P = e->prof;
        if (P && pass == 1) d.prof_chunks++;   // chunks, not passes: a Lynch run formats each chunk again in pass 2
        if (!pre_tiled) {
            W.lens_ready = false;   // (set by this chunk's parse when it computes the -m local record lengths)
            W.cls_ready = false;    // (... and the class words)
        }
        const uint64_t tbytes = L.c1 - (L.c0 & ~(uint64_t)15);
        if (x == hipSuccess && !pre_indexed && !pre_tiled) rc = sid_chunk_reserve(&W, tbytes, 0);
        const bool lynch_hist = pass == 1 && e->lynch;
        const bool format = pass == 2 || (needs_format_pass1(e) && (!d.hold_full.load() || sink_all_pass1(e)));
        // -m local / quality (and pass 2 of the Lynch paths): call, then the
        // one-pass formatter into a buffer of the records' upper bound -- the
        // device's hold arena in pass 1 (committed to the exact bytes after),
        // else a pooled scratch buffer
        char* out = nullptr;
        uint64_t cap = 0;   // 0: arena memory (never returned to the pool)
        bool via_host = false;   // pass 1: records go on to the host arena (a pooled device buffer meanwhile)
        bool sunk = false;       // pass 1, device sink: a scratch buffer, dropped
        hipEvent_t pe = nullptr;
        uint64_t n = 0;
        StageSets sets = pre_tiled ? next_sets : StageSets{};   // the stages' sets of this chunk (none: no stage ran)
        // the tile path: this chunk's records and byte count done (recorded
        // before the next chunk's tile parse is queued behind the writer: the
        // host and the records' D2H wait for this, not for that parse, which
        // waits for the next chunk's upload -- each chunk's D2H then runs
        // behind its own writer instead of a chunk later)
        struct Done {
            Dev& d;
            hipEvent_t ev = nullptr;
            void drop()
            {
                if (ev) d.give_event(ev);
                ev = nullptr;
            }
            ~Done() { drop(); }
        } done{d};
        // -m local formatting in this pass, lines of up to 256 B on average (as
        // the device's last chunk had): the tile parse -- the text read once,
        // no host round trip before the writer (sid_chunk_tile_local).  A tile
        // with more lines than its slots sends the chunk again through the
        // two-pass path below (its records dropped), the next chunks with
        // more slots
        // (pre_tiled: this chunk's tile parse already ran behind the previous
        // chunk's writer, with the slots and shape of that time)
        bool tiled = false;
        const bool tile_was_off = !d.tile_ok;   // (this chunk then goes the two-pass way, and may turn it on)
        const bool tile_path =x == hipSuccess && rc == SID_OK && format && !lynch_hist && !qmode &&
                               (d.tile_ok || pre_tiled) && e->opts.method == SID_METHOD_LOCAL &&
                               sid_chunk_local_ok(d.ctx) && !(pass == 2 && r.pre);
        if (pre_tiled && !tile_path) {
            W.slot_cap = 0;   // (its slots unused: the dense layout again)
            pre_tiled = false;
        }
        if (tile_path) {
            const uint32_t lg = pre_tiled ? next_lg : d.tile_cap;
            const bool quad = pre_tiled ? next_quad : d.tile_quad;
            if (!pre_tiled) rc = sid_chunk_reserve(&W, tbytes, sid_chunk_tile_slots(L.c0, L.c1, lg, quad));
            if (rc != SID_OK) return (void)fail(e, rc);
            // (VCF lines: their own bound, wherever a chunk's records are reserved -- the hold arena, the
            // pooled buffers on the way to the host arena, the device sink's and pass 2's)
            const uint64_t bound = W.vcf ? sid_chunk_vcf_bound(sid_chunk_tile_slots(L.c0, L.c1, lg, quad), L.c1 - L.c0)
                                         : sid_chunk_tile_bound(L.c0, L.c1, lg, quad);
            // the records' buffer, taken as the two-pass path below takes it
            // (near the hold budget that path decides, with its exact bound)
            if (pass == 1 && d.hh && !d.hh_full) {
                out = d.pool.get(bound, &cap, d.s_comp);
                via_host = out != nullptr;
                if (!out) cap = 0;
            }
            if (via_host) {
            } else if (pass == 1 && sink_all_pass1(e)) {
                out = d.pool.get(bound, &cap, d.s_comp);
                sunk = out != nullptr;
                if (!out) cap = 0;
            } else if (pass == 1 && d.hold_used.load() + bound > d.hold_budget) {
            } else if (pass == 1) {
                out = d.arena_reserve(bound, d.hold_budget - d.hold_used.load());
            } else {
                out = d.pool.get(bound, &cap, d.s_comp);
                if (!out) cap = 0;
            }
            if (!out && pre_tiled) {
                W.slot_cap = 0;
                pre_tiled = false;
            }
            if (out) {
                if (!pre_tiled) {
                    pe = d.prof_begin(P);
                    rc = sid_chunk_tile_local(d.ctx, &W, L.base, L.c0, L.c1, lg, quad, e->conf_type, d.s_comp);
                    d.prof_end(1, pe);
                    sets = stage_sets(W);
                }
                if (rc == SID_OK) {
                    pe = d.prof_begin(P);
                    rc = sid_chunk_local_put(d.ctx, &W, L.base, L.c1, 0, e->conf_type, out, d.s_comp);
                    d.prof_end(5, pe);
                }
                W.slot_cap = 0;   // (the workspace's dense layout again for the two-pass path)
                if (rc != SID_OK) return (void)fail(e, rc);
                // bytes, range flag, sites, parse error key, the most lines in a tile
                x = hipMemcpyAsync(hs + 8, W.lb + 1, 5 * 8, hipMemcpyDeviceToHost, d.s_comp);
                if (x == hipSuccess && e->cx_on)
                    x = hipMemcpyAsync(d.h_cx, W.cx_desc, sizeof(sid_cx_desc), hipMemcpyDeviceToHost, d.s_comp);
                if (x == hipSuccess && (done.ev = d.take_event())) x = hipEventRecord(done.ev, d.s_comp);
                // the next chunk's tile parse behind this writer (stream order:
                // it rewrites the slots and W.lb after the writer and the copy
                // have read them), so the GPU does not idle over the host round
                // trip; with this chunk's slots and shape (a change takes effect
                // a chunk later), dropped if this chunk overflows
                if (x == hipSuccess && !have_next && d.loaded.try_pop(nextL)) {
                    have_next = true;
                    const ChunkRec& r2 = e->recs[nextL.j];
                    if (nextL.kind == 0 && !(pass == 2 && r2.pre) && !(pass == 1 && nextL.j > e->first_err.load())) {
                        d.tile_ahead(nextL.lines, nextL.lbytes);
                        const uint32_t lg2 = d.tile_cap;
                        const bool q2 = d.tile_quad;
                        if (nextL.ev) x = hipStreamWaitEvent(d.s_comp, nextL.ev, 0);
                        int rc2 = SID_OK;
                        // growth frees buffers: hipFree waits for the queued work first
                        if (x == hipSuccess)
                            rc2 = sid_chunk_reserve(&W, nextL.c1 - (nextL.c0 & ~(uint64_t)15),
                                                    sid_chunk_tile_slots(nextL.c0, nextL.c1, lg2, q2));
                        hipEvent_t pe2 = d.prof_begin(P);
                        if (rc2 == SID_OK && x == hipSuccess)
                            rc2 = sid_chunk_tile_local(d.ctx, &W, nextL.base, nextL.c0, nextL.c1, lg2, q2,
                                                       e->conf_type, d.s_comp);
                        d.prof_end(1, pe2);
                        if (rc2 != SID_OK) return (void)fail(e, rc2);
                        next_tiled = x == hipSuccess;
                        next_sets = stage_sets(W);
                        next_lg = lg2;
                        next_quad = q2;
                    }
                }
                if (x == hipSuccess) x = done.ev ? sync_ev(done.ev) : sync();
                if (x != hipSuccess) return (void)hipfail(e, x);
                const uint64_t maxl = hs[12];
                // (rows or names beyond the stage's set: the two-pass path sizes it; the next chunks' sets grow)
                const bool win_over = windows && maxl <= lg && !win_fits(sets.win);
                if (win_over) win_want(sets.win);
                if (maxl <= lg && !win_over) {
                    tiled = true;
                    ++d.tiled;
                    n = hs[10];
                    r.parsed = n;
                    hs[4] = hs[11];
                    // the next chunk's shape and slots (a new shape: from this
                    // chunk's lines per byte, a quarter on top)
                    d.tile_next(maxl, n, L.c1 - L.c0, quad);
                } else {
                    if (cap) d.pool.put(out, cap, d.s_comp);
                    out = nullptr;
                    cap = 0;
                    via_host = sunk = false;
                    done.drop();
                    if (!win_over) {
                        ++d.tile_overflows;
                        d.tile_over_queued += have_next;
                        d.tile_over(maxl, quad);
                    }
                    // this chunk goes the two-pass way through the workspace:
                    // the next chunk's tile parse is dropped (it runs again)
                    W.slot_cap = 0;
                    next_tiled = false;
                }
            }
        }
        // The Lynch paths' first pass likewise: the tile parse into every
        // site's counts and header pair, compacted into the buffer kept for
        // pass 2 (the two-pass parse's layout), then the histogram.  Without
        // room for that buffer (the retain budget), the two-pass path below
        // (pass 2 then indexes and parses the text again).
        if (!tiled && x == hipSuccess && rc == SID_OK && lynch_hist && !qmode && d.tile_ok) {
            const uint32_t cp = d.tile_cap;
            const bool quad = d.tile_quad;
            rc = sid_chunk_reserve(&W, tbytes, sid_chunk_tile_slots(L.c0, L.c1, cp, quad));
            if (rc != SID_OK) return (void)fail(e, rc);
            pe = d.prof_begin(P);
            rc = sid_chunk_tile_counts(&W, L.base, L.c0, L.c1, cp, quad, d.s_comp);
            if (rc != SID_OK) return (void)fail(e, rc);
            x = hipMemcpyAsync(hs, W.state, 8, hipMemcpyDeviceToHost, d.s_comp);   // sites
            if (x == hipSuccess) x = hipMemcpyAsync(hs + 4, W.state + 4, 8, hipMemcpyDeviceToHost, d.s_comp);
            if (x == hipSuccess) x = hipMemcpyAsync(hs + 12, W.lb + 5, 8, hipMemcpyDeviceToHost, d.s_comp);
            if (x == hipSuccess) x = sync();
            if (x != hipSuccess) return (void)hipfail(e, x);
            const uint64_t maxl = hs[12], m = hs[0];
            if (maxl > cp) {   // a tile with more lines than slots: the two-pass path
                W.slot_cap = 0;
                d.prof_end(1, pe);
                ++d.tile_overflows;
                d.tile_over(maxl, quad);
            } else {
                const uint64_t m2 = (m + 1) & ~(uint64_t)1, m4 = (m + 3) & ~(uint64_t)3;
                // (sid_opts.variants: the sites' reference bytes behind the header pairs, 1 B a site)
                const uint64_t pre_bytes = 4 * m4 + 24 * m2 + (W.refb ? m : 0);
                uint64_t pc = 0;
                char* pre = m && d.retain_used.load() + pre_bytes <= d.retain_budget
                                ? d.pool.get(pre_bytes, &pc, d.s_comp) : nullptr;
                if (m == 0 || pre) {
                    uint64_t* counts = nullptr;
                    if (pre) {
                        r.pre = pre;
                        r.pre_cap = pc;
                        d.retain_used += pc;
                        counts = (uint64_t*)(pre + 4 * m4);
                        rc = sid_chunk_tile_compact(&W, (sid_off_t*)pre, counts, counts + m2,
                                                    W.refb ? (uint8_t*)(counts + 3 * m2) : nullptr, d.s_comp);
                        if (rc != SID_OK) return (void)fail(e, rc);
                    }
                    W.slot_cap = 0;
                    d.prof_end(1, pe);
                    n = m;
                    r.parsed = n;
                    pe = d.prof_begin(P);
                    rc = sid_profile_accumulate(d.ctx, (const uint16_t*)counts, n, d.s_comp);   // synchronises
                    d.prof_end(3, pe);
                    if (rc == SID_OK && n == 0) x = sync();
                    if (rc != SID_OK) return (void)fail(e, rc);
                    if (x != hipSuccess) return (void)hipfail(e, x);
                    tiled = true;
                    ++d.tiled;
                    d.tile_next(maxl, n, L.c1 - L.c0, quad);
                } else {
                    W.slot_cap = 0;   // no room to keep the parse: the two-pass path
                    d.prof_end(1, pe);
                }
            }
        }
        if (!tiled) {
        // pass 2 of a Lynch path: the parse kept since pass 1 stands in for the
        // workspace's line offsets, counts and header pairs (restored below)
        struct View {
            sid_chunk_ws& W;
            sid_off_t* starts;
            uint64_t *counts, *hdr;
            uint8_t* refb;
            bool on = false;
            ~View()
            {
                if (on) W.starts = starts, W.counts = counts, W.hdr = hdr, W.refb = refb;
            }
        } view{W, W.starts, W.counts, W.hdr, W.refb};
        // the kept parse's layout: starts (4 B), counts (8 B), header pairs
        // (16 B), each at a 16-B aligned offset (the lookup reads counts as
        // 16-B site pairs), then with sid_opts.variants the reference bytes
        // (1 B; the workspace has an array of them exactly then)
        auto use_pre = [&](char* pre, uint64_t m) {
            view.starts = W.starts, view.counts = W.counts, view.hdr = W.hdr, view.refb = W.refb, view.on = true;
            const uint64_t m2 = (m + 1) & ~(uint64_t)1, m4 = (m + 3) & ~(uint64_t)3;
            W.starts = (sid_off_t*)pre;
            W.counts = (uint64_t*)(pre + 4 * m4);
            W.hdr = W.counts + m2;
            if (W.refb) W.refb = (uint8_t*)(W.hdr + 2 * m2);
        };
        if (pass == 2 && r.pre) {
            n = r.parsed;
            rc = sid_chunk_reserve(&W, 0, n);
            if (rc != SID_OK) return (void)fail(e, rc);
            use_pre(r.pre, n);
            if (x == hipSuccess) x = hipMemsetAsync(W.state + 4, 0xFF, sizeof(uint64_t), d.s_comp);   // no parse error
            if (x != hipSuccess) return (void)hipfail(e, x);
        } else {
            if (!pre_indexed) {
                pe = d.prof_begin(P);
                if (rc == SID_OK && x == hipSuccess) rc = sid_chunk_index(&W, L.base, L.c0, L.c1, d.s_comp);
                d.prof_end(0, pe);
                if (rc == SID_OK && x == hipSuccess) x = hipMemcpyAsync(hs, W.state, 8, hipMemcpyDeviceToHost, d.s_comp);
                if (rc == SID_OK && x == hipSuccess) x = sync();
            }
            if (x != hipSuccess) return (void)hipfail(e, x);
            if (rc != SID_OK) return (void)fail(e, rc);
            n = hs[0];
            rc = sid_chunk_reserve(&W, 0, n);
            if (rc != SID_OK) return (void)fail(e, rc);
            r.parsed = n;
            if (tile_was_off && !qmode) d.tile_retry(n, L.c1 - L.c0);
            // Lynch paths: the parse goes straight into a buffer kept for
            // pass 2 (which then skips index and parse) while the retain
            // budget allows: 28 B a site, cheaper than indexing and parsing
            // the text again
            const uint64_t pre_bytes = 4 * ((n + 3) & ~(uint64_t)3) + 24 * ((n + 1) & ~(uint64_t)1) + (W.refb ? n : 0);
            if (pass == 1 && e->lynch && n && !qmode && d.retain_used.load() + pre_bytes <= d.retain_budget) {
                uint64_t pc = 0;
                char* pre = d.pool.get(pre_bytes, &pc, d.s_comp);
                if (pre) {
                    r.pre = pre;
                    r.pre_cap = pc;
                    d.retain_used += pc;
                    use_pre(pre, n);
                }
            }
            pe = d.prof_begin(P);
            // -m local: the records' lengths come out of the parse when this
            // pass formats (sid_parse_len_kernel; the length kernel is skipped)
            const bool lens = e->opts.method == SID_METHOD_LOCAL && sid_chunk_local_ok(d.ctx) && !qmode &&
                              !(pass == 1 && e->lynch) && (pass == 2 || needs_format_pass1(e));
            if (rc == SID_OK) rc = sid_chunk_parse(&W, L.base, L.c0, L.c1, n, qmode, d.s_comp, lens ? d.ctx : nullptr);
            d.prof_end(1, pe);
            if (rc != SID_OK) return (void)fail(e, rc);
        }
        if (lynch_hist) {
            x = hipMemcpyAsync(hs + 4, W.state + 4, 8, hipMemcpyDeviceToHost, d.s_comp);
            if (x != hipSuccess) return (void)hipfail(e, x);
            pe = d.prof_begin(P);
            rc = sid_profile_accumulate(d.ctx, (const uint16_t*)W.counts, n, d.s_comp);   // synchronises
            d.prof_end(3, pe);
            if (rc == SID_OK && n == 0) x = sync();
            if (rc != SID_OK) return (void)fail(e, rc);
            if (x != hipSuccess) return (void)hipfail(e, x);
        }
        // -m local: the call fused into the formatter (sid_chunk_local_*)
        const bool fused = e->opts.method == SID_METHOD_LOCAL && sid_chunk_local_ok(d.ctx);
        // likelihood_ratio / bayes pass 2: the class lookup fused into the
        // formatter (sid_chunk_lynch_*; the records' tails prebuilt per class)
        sid_lynch_fmt lv;
        const bool lfused = pass == 2 && !fused && sid_lynch_fmt_view(d.ctx, &lv) == SID_OK;
        if (format && !lynch_hist) {
            if (!fused && !lfused) {
                pe = d.prof_begin(P);
                rc = call_sites(e, d, L, n);
                d.prof_end(2, pe);
                if (rc != SID_OK) return (void)fail(e, rc);
            }
            const uint64_t bound = W.vcf ? sid_chunk_vcf_bound(n, L.c1 - L.c0) : sid_chunk_fmt_bound(n, L.c1 - L.c0);
            if (n && pass == 1 && d.hh && !d.hh_full) {
                out = d.pool.get(bound, &cap, d.s_comp);
                via_host = out != nullptr;
                if (!out) cap = 0;
            }
            if (n == 0 || via_host) {
            } else if (pass == 1 && sink_all_pass1(e)) {
                // (no hold arena: nothing is emitted, so no record need wait
                // in HBM; the pooled buffer is reused chunk after chunk)
                out = d.pool.get(bound, &cap, d.s_comp);
                sunk = out != nullptr;   // (no HBM for it: formatted in pass 2 instead)
                if (!out) cap = 0, d.hold_full = true;
            } else if (pass == 1 && d.hold_used.load() + bound > d.hold_budget) {
                d.hold_full = true;   // this chunk and the rest: formatted in pass 2
            } else if (pass == 1) {
                // no HBM for the arena: formatted in pass 2 instead
                if (!(out = d.arena_reserve(bound, d.hold_budget - d.hold_used.load()))) d.hold_full = true;
            } else {
                if (!(out = d.pool.get(bound, &cap, d.s_comp))) return (void)fail(e, SID_ENOMEM);
            }
            if (out) {
                pe = d.prof_begin(P);
                rc = fused    ? sid_chunk_local_len(d.ctx, &W, L.base, L.c1, n, e->conf_type, d.s_comp)
                     : lfused ? sid_chunk_lynch_len(d.ctx, &W, L.base, L.c1, n, d.s_comp)
                              : sid_chunk_fmt_len(&W, L.base, L.c1, n, e->conf_type, d.s_comp);
                d.prof_end(4, pe);
                if (rc != SID_OK) return (void)fail(e, rc);
                sets = stage_sets(W);
                pe = d.prof_begin(P);
                rc = fused    ? sid_chunk_local_put(d.ctx, &W, L.base, L.c1, n, e->conf_type, out, d.s_comp)
                     : lfused ? sid_chunk_lynch_put(d.ctx, &W, L.base, L.c1, n, out, d.s_comp)
                              : sid_chunk_fmt_put(&W, L.base, L.c1, n, e->conf_type, out, d.s_comp);
                d.prof_end(5, pe);
                if (rc != SID_OK) return (void)fail(e, rc);
                x = hipMemcpyAsync(hs + 8, W.lb + 1, 32, hipMemcpyDeviceToHost, d.s_comp);   // bytes, flags, error
                if (x == hipSuccess && e->cx_on)
                    x = hipMemcpyAsync(d.h_cx, W.cx_desc, sizeof(sid_cx_desc), hipMemcpyDeviceToHost, d.s_comp);
                // the next chunk's line index behind the formatter (stream
                // order: it rewrites W.state only after the formatter has read it)
                // (not when the tile path already took the next chunk: this
                // chunk overflowed its slots and came here)
                if (x == hipSuccess && !have_next && d.loaded.try_pop(nextL)) {
                    have_next = true;
                    const ChunkRec& r2 = e->recs[nextL.j];
                    if (nextL.kind == 0 && !(pass == 2 && r2.pre) && !(pass == 1 && nextL.j > e->first_err.load())) {
                        if (nextL.ev) x = hipStreamWaitEvent(d.s_comp, nextL.ev, 0);
                        int rc2 = SID_OK;
                        // growth frees buffers: hipFree waits for the queued work first
                        if (x == hipSuccess) rc2 = sid_chunk_reserve(&W, nextL.c1 - (nextL.c0 & ~(uint64_t)15), 0);
                        hipEvent_t pe2 = d.prof_begin(P);
                        if (rc2 == SID_OK && x == hipSuccess)
                            rc2 = sid_chunk_index(&W, nextL.base, nextL.c0, nextL.c1, d.s_comp);
                        d.prof_end(0, pe2);
                        if (rc2 == SID_OK && x == hipSuccess)
                            x = hipMemcpyAsync(hs, W.state, 8, hipMemcpyDeviceToHost, d.s_comp);
                        if (rc2 != SID_OK) return (void)fail(e, rc2);
                        next_indexed = x == hipSuccess;
                    }
                }
                if (x == hipSuccess) x = sync();
                if (x != hipSuccess) return (void)hipfail(e, x);
                hs[4] = hs[11];
            }
        }
        }   // (the two-pass path)
        if (!lynch_hist && !out) {
            x = hipMemcpyAsync(hs + 4, W.state + 4, 8, hipMemcpyDeviceToHost, d.s_comp);
            if (x == hipSuccess) x = sync();
            if (x != hipSuccess) return (void)hipfail(e, x);
            hs[8] = 0;
        }
        const uint64_t err = hs[4];
        if (err != ~0ull) {   // a malformed line: the rest of the input is moot
            r.err = err - 8 * L.c0;
            if (out && cap) d.pool.put(out, cap, d.s_comp);
            uint64_t cur = e->first_err.load();
            while (L.j < cur && !e->first_err.compare_exchange_weak(cur, L.j)) {
            }
            release_slot();
            if (pass == 2) return (void)fail(e, SID_EMALFORMED);   // cannot happen: pass 1 validated
            continue;
        }
        if (pass == 1 && n == 0 && format && !lynch_hist) {
            // a chunk without sites has no records: done in pass 1 for the
            // sinks that take records then (else the emit would start its
            // threads and a second pass for it)
            if (sink_all_pass1(e)) {
                r.sunk = true;
                r.held_len = 0;
            } else if (d.hh) {
                r.host = d.hh;
                r.host_len = 0;
                r.host1 = true;
            }
        }
        if (!format || lynch_hist || (pass == 1 && !out)) {
            release_slot();
            continue;
        }
        if (out && hs[9]) return (void)fail(e, SID_ERANGE);
        const uint64_t bytes = hs[8];
        if (e->cx_on) {   // (read back by the sync that brought the byte count)
            r.cx = out ? *d.h_cx : sid_cx_desc{};   // (a chunk without sites: nothing ran, nothing to stitch)
            r.cx_total = bytes;
        }
        if (windows) {   // (likewise; a chunk without sites: no stage ran, no row)
            r.win.clear();
            if (out) {
                if (sets.win < 0 || !win_fits(sets.win)) return (void)fail(e, SID_ESTATE);   // (the two-pass stage sized its set)
                win_want(sets.win);
                x = win_take(sets.win, r.win);
                if (x != hipSuccess) return (void)hipfail(e, x);
            }
        }
        if (dhist) {   // (likewise)
            r.dh.clear();
            if (out) {
                if (sets.dh < 0) return (void)fail(e, SID_ESTATE);
                x = bins_take(W.dh, sets.dh, SID_DH_BINS, SID_DH_EAGER_ROWS, r.dh, d.s_comp, sync);
                if (x != hipSuccess) return (void)hipfail(e, x);
                if (!sid_dh_sort(&r.dh)) return (void)fail(e, SID_ESTATE);
            }
        }
        if (rstats) {   // (likewise)
            r.rs.clear();
            if (out) {
                if (sets.rs < 0) return (void)fail(e, SID_ESTATE);
                x = bins_take(W.rs, sets.rs, W.rs.n, SID_RS_EAGER_ROWS, r.rs, d.s_comp, sync);
                if (x != hipSuccess) return (void)hipfail(e, x);
                if (!sid_rs_check(r.rs, W.rs.n)) return (void)fail(e, SID_ESTATE);
            }
        }
        release_slot();
        if (pass == 2 && r.kept) {   // kept text done with: back to the pool after this stream's work
            d.pool.put(r.kept, r.kept_cap, d.s_comp);
            r.kept = nullptr;
        }
        if (pass == 2 && r.pre) {
            d.pool.put(r.pre, r.pre_cap, d.s_comp);
            r.pre = nullptr;
        }
        if (pass == 1 && sunk) {
            r.sunk = true;
            r.held_len = bytes;
            d.pool.put(out, cap, d.s_comp);   // reused on this stream only: ordered
            continue;
        }
        if (pass == 1 && via_host) {
            char* hp = d.hh_take(bytes);
            if (hp) {   // D2H behind this chunk's formatter, while the next chunks upload
                hipEvent_t ev = done.ev ? nullptr : d.take_event();
                if (!done.ev && !ev) return (void)fail(e, SID_EHIP);
                if (ev) x = hipEventRecord(ev, d.s_comp);
                if (x == hipSuccess) x = hipStreamWaitEvent(d.s_d2h, ev ? ev : done.ev, 0);
                if (ev) d.give_event(ev);
                if (x == hipSuccess && bytes) x = hipMemcpyAsync(hp, out, bytes, hipMemcpyDeviceToHost, d.s_d2h);
                if (x != hipSuccess) return (void)hipfail(e, x);
                d.pool.put(out, cap, d.s_d2h);   // reusable once the copy is done
                r.host = hp;
                r.host_len = bytes;
                r.host1 = true;
                continue;
            }
            // the host arena is full: keep the records on the device while
            // the hold budget allows, else format the chunk again in pass 2
            d.hh_full = true;
            if (d.hold_used.load() + cap <= d.hold_budget) {
                r.held = out;
                r.held_cap = cap;
                r.held_len = bytes;
                d.hold_used += cap;
            } else {
                d.hold_full = true;
                d.pool.put(out, cap, d.s_comp);
            }
            continue;
        }
        if (pass == 1) {
            d.arena_commit(bytes);
            r.held = out;
            r.held_cap = 0;
            r.held_len = bytes;
            d.hold_used += (bytes + 255) & ~(uint64_t)255;
            continue;
        }
        if (e->cfg.device_sink == 1) {
            e->sink_bytes += bytes;
            d.pool.put(out, cap, nullptr);   // reused on this stream only: ordered
            continue;
        }
        OutItem it;
        it.j = L.j;
        it.buf = out;
        it.cap = cap;
        it.len = bytes;
        hipEvent_t ev = done.ev;
        done.ev = nullptr;
        if (!ev) {
            if (!(ev = d.take_event())) return (void)fail(e, SID_EHIP);
            (void)hipEventRecord(ev, d.s_comp);
        }
        it.ev = ev;
        if (!d.drain_q.push(it)) break;
    }
    W.slot_cap = 0;   // (a tile parse run ahead for a chunk this pass then skipped)
    if (pass == 2) d.drain_q.close();
}

// the drain of device d: CSV buffers through the pinned ring to the writer
void drain(sid_engine* e, Dev& d)
{
    bind_thread(d);
    if (hipSetDevice(d.device) != hipSuccess) return (void)fail(e, SID_EHIP);
    OutItem it;
    while (d.drain_q.pop(it)) {
        if (e->rc.load() != SID_OK) break;
        hipError_t x = hipSuccess;
        if (it.ev) {
            x = hipStreamWaitEvent(d.s_d2h, it.ev, 0);
            // free again once the wait is enqueued: the wait is on the record
            // made before it, a later record does not affect it
            d.give_event(it.ev);
        }
        if (x != hipSuccess) return (void)hipfail(e, x);
        if (it.len == 0) {
            if (d.hh) e->recs[it.j].host = d.hh, e->recs[it.j].host_len = 0;
            Piece p;
            p.j = it.j;
            p.last = true;
            p.buf = it.buf;
            p.cap = it.cap;
            if (!d.out_q.push(p)) break;
            continue;
        }
        if (char* hp = d.hh_take(it.len)) {   // the whole chunk into the host arena, one copy
            hipEvent_t ev = d.take_event();
            if (!ev) return (void)fail(e, SID_EHIP);
            x = hipMemcpyAsync(hp, it.buf, it.len, hipMemcpyDeviceToHost, d.s_d2h);
            if (x == hipSuccess) x = hipEventRecord(ev, d.s_d2h);
            if (x != hipSuccess) return (void)hipfail(e, x);
            e->recs[it.j].host = hp;
            e->recs[it.j].host_len = it.len;
            Piece p;
            p.j = it.j;
            p.len = it.len;
            p.last = true;
            p.buf = it.buf;
            p.cap = it.cap;
            p.host = hp;
            p.hev = ev;
            if (!d.out_q.push(p)) return;
            continue;
        }
        for (uint64_t o = 0; o < it.len;) {
            int ps;
            if (!d.free_pinned.pop(ps)) return;
            const uint64_t m = std::min<uint64_t>(d.pinned_cap, it.len - o);
            x = hipMemcpyAsync(d.pinned[ps], it.buf + o, m, hipMemcpyDeviceToHost, d.s_d2h);
            if (x == hipSuccess) x = hipEventRecord(d.pinned_ev[ps], d.s_d2h);
            if (x != hipSuccess) return (void)hipfail(e, x);
            o += m;
            Piece p;
            p.j = it.j;
            p.ps = ps;
            p.len = m;
            p.last = o == it.len;
            if (p.last) {
                p.buf = it.buf;
                p.cap = it.cap;
            }
            if (!d.out_q.push(p)) return;
        }
    }
    d.out_q.close();
}

// The writer under a context (sid_opts.context): a chunk's bytes arrive in
// file order, in pieces; the records between its two forced zones and the
// head zone's (decided by the chunks in front) go out at once, the tail zone's
// bytes (at most N records) are held until the stitch has seen enough of the
// chunks behind to decide them -- the next chunk, as a rule.
struct CxWriter {
    sid_engine* e;
    sid_write_fn write;
    void* user;
    sid_cx_stitch S;
    std::vector<std::string> held;   // per chunk: its tail zone's bytes
    size_t flushed = 0;              // the chunks whose held bytes are decided and written
    size_t complete = 0;             // the chunks whose bytes have all arrived
    bool ok = true;
    const ChunkRec* r = nullptr;     // the chunk arriving
    uint64_t pos = 0, t0 = 0;        // bytes of it seen; its tail zone starts at t0
    sid_cx_range rg[2 * SID_CONTEXT_MAX + 1];
    size_t nr = 0;

    CxWriter(sid_engine* e_, sid_write_fn w, void* u) : e(e_), write(w), user(u), S(e_->cx_n), held(e_->recs.size()) {}
    void put(const char* p, uint64_t len)
    {
        if (ok && len && write(user, p, len) != 0) ok = false;
    }
    void flush()
    {
        for (; flushed < std::min(S.resolved(), complete); ++flushed) {
            const ChunkRec& c = e->recs[flushed];
            std::string& h = held[flushed];
            if (h.empty()) continue;
            sid_cx_range g[2 * SID_CONTEXT_MAX + 1];
            const uint64_t c0 = c.cx_total - h.size();
            const size_t n = sid_cx_ranges(c.cx, e->cx_n, S.verdict(flushed), c.cx_total, g, nullptr);
            for (size_t k = 0; k < n; ++k) {
                const uint64_t a = std::max(g[k].off, c0), b = g[k].off + g[k].len;
                if (b > a) put(h.data() + (a - c0), b - a);
            }
            std::string().swap(h);
        }
    }
    void begin(uint64_t j)
    {
        r = &e->recs[j];
        S.push(r->cx);
        complete = j;   // (the chunks in front of it)
        flush();
        pos = 0;
        uint64_t tail = 0;
        for (uint32_t k = 0; k < sid_cx_zone(r->cx, e->cx_n); ++k) tail += r->cx.tail_len[k];
        t0 = r->cx_total - std::min(tail, r->cx_total);
        nr = sid_cx_ranges(r->cx, e->cx_n, S.verdict(j), r->cx_total, rg, nullptr);
        held[j].reserve(r->cx_total - t0);
    }
    // the chunk's next bytes
    void piece(uint64_t j, const char* p, uint64_t len)
    {
        const uint64_t lo = pos, hi = pos + len;
        for (size_t k = 0; k < nr; ++k) {   // in front of the tail zone: decided
            const uint64_t a = std::max(rg[k].off, lo), b = std::min({rg[k].off + rg[k].len, hi, t0});
            if (b > a) put(p + (a - lo), b - a);
        }
        if (hi > t0) {
            const uint64_t a = std::max(lo, t0);
            held[j].append(p + (a - lo), hi - a);
        }
        pos = hi;
    }
    void finish()
    {
        S.finish();
        complete = S.chunks();
        flush();
    }
};

// After the emit under a context: every chunk's final verdicts (all the
// descriptors are there), the bytes they keep -- the run's bytes_out in every
// sink mode -- and the chunks in the host arena cut down to them in place
// (sid_engine_records).
uint64_t cx_settle(sid_engine* e)
{
    sid_cx_stitch S(e->cx_n);
    for (const auto& r : e->recs) S.push(r.cx);
    S.finish();
    uint64_t out = 0;
    sid_cx_range g[2 * SID_CONTEXT_MAX + 1];
    for (size_t j = 0; j < e->recs.size(); ++j) {
        ChunkRec& r = e->recs[j];
        uint64_t kept = 0;
        const size_t n = sid_cx_ranges(r.cx, e->cx_n, S.verdict(j), r.cx_total, g, &kept);
        out += kept;
        if (r.host && r.host_len == r.cx_total) r.host_len = sid_cx_compact(const_cast<char*>(r.host), g, n);
    }
    return out;
}

}  // namespace

// ------------------------------------------------------------------ phases --
static void timing_report(sid_engine* e, const char* phase, double s)
{
    static const bool on = std::getenv("SID_ENGINE_TIMING") != nullptr;
    if (on)
        std::fprintf(stderr,
                     "{\"engine_phase\": \"%s\", \"s\": %.6f, \"compute_sync_s\": %.6f, \"writer_wait_s\": %.6f, "
                     "\"chunks_registered\": %llu, \"strip_threads\": %d, \"strip_busy_s\": %.6f, "
                     "\"strip_busy_min_s\": %.6f, \"strip_busy_max_s\": %.6f, "
                     "\"chunks_stripped\": %llu, \"strip_bytes\": %llu, \"h2d_bytes\": %llu}\n",
                     phase, s, e->t_comp_sync.load() * 1e-9, e->t_write_wait.load() * 1e-9,
                     (unsigned long long)e->reg_chunks.load(), e->strip_T, e->t_strip.load() * 1e-9,
                     e->t_strip_max.load() ? e->t_strip_min.load() * 1e-9 : 0.0, e->t_strip_max.load() * 1e-9,
                     (unsigned long long)e->strip_chunks.load(), (unsigned long long)e->strip_bytes.load(),
                     (unsigned long long)e->last_h2d_bytes);
    e->t_comp_sync = e->t_write_wait = 0;
    e->reg_chunks = 0;
    e->t_register = 0;
}

static void reset_run(sid_engine* e)
{
    e->rc = SID_OK;
    e->first_err = UINT64_MAX;
    const int m = e->opts.method;
    e->quality = m == SID_METHOD_QUALITY;
    e->lynch = m == SID_METHOD_LIKELIHOOD_RATIO || m == SID_METHOD_BAYES || e->opts.estimate_prior;
    e->conf_type = m == SID_METHOD_BAYES ? "probability" : "p_value";
    for (auto& r : e->recs) {
        Dev& d = *e->devs[r.dev];
        if (r.held) d.pool.put(r.held, r.held_cap, nullptr);
        if (r.kept) d.pool.put(r.kept, r.kept_cap, nullptr);
        if (r.pre) d.pool.put(r.pre, r.pre_cap, nullptr);
        r.held = r.kept = r.pre = nullptr;
        r.held_len = r.kept_len = 0;
        r.host = nullptr;
        r.host_len = 0;
        r.host1 = false;
        r.sunk = false;
        r.err = ~0ull;
        r.zbad = ~0ull;
        r.smap.clear();
        r.parsed = 0;
        r.cx = sid_cx_desc{};
        r.cx_total = 0;
        r.win.clear();
        r.dh.clear();
        r.rs.clear();
    }
    e->win.clear();
    e->win_ready = false;
    e->dh.clear();
    e->dh_ready = false;
    sid_region_stats_free(e->rs);
    e->rs = nullptr, e->rs_n = 0;
    e->rs_ready = false;
    e->z_bytes = 0;
    e->z_blocks = 0;
    e->strip_chunks = 0;
    e->strip_bytes = 0;
    e->t_strip = 0;
    e->t_strip_min = UINT64_MAX;
    e->t_strip_max = 0;
    for (auto& dp : e->devs) {
        Dev& d = *dp;
        d.hold_used = 0;
        d.retain_used = 0;
        d.hold_full = false;
        d.arena_seg = 0;
        d.arena_off = 0;
        d.hh_off = 0;
        d.hh_full = false;
        (void)d.h2d_collect();   // (a failed run's copies: its devices were synchronised)
        d.h2d_bytes = 0;
        d.tiled = d.tile_overflows = d.tile_over_queued = 0;
        d.tile_reset();
        d.ws.slot_cap = 0;   // (a failed run may leave the slot layout set)
    }
    e->hist_merged = false;
}

static void start_queues(sid_engine* e)
{
    for (auto& dp : e->devs) {
        Dev& d = *dp;
        d.free_slots.reset();
        d.loaded.reset();
        d.drain_q.reset();
        d.out_q.reset();
        d.free_pinned.reset();
        for (int s = 0; s < (int)d.slots.size(); ++s) d.free_slots.push(s);
    }
}

static int setup_budgets(sid_engine* e)
{
    for (auto& dp : e->devs) {
        Dev& d = *dp;
        if (hipSetDevice(d.device) != hipSuccess) return SID_EHIP;
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) return SID_EHIP;
        const uint64_t avail = fr + d.pool.bytes() + d.arena_bytes();   // pooled buffers and the arena are reusable
        // the GPU's pipelines share its memory (avail: what this one sees free)
        const double share = 0.40 / std::max(1, e->cfg.lanes);
        d.hold_budget = e->cfg.hold_bytes ? e->cfg.hold_bytes : (uint64_t)(avail * share);
        d.retain_budget = e->cfg.retain_bytes ? e->cfg.retain_bytes : (uint64_t)(avail * share);
        // the host arena: pinned (and so populated) once, reused by every run
        const uint64_t hb = e->cfg.device_sink == 1 ? 0 : e->cfg.host_hold_bytes;
        if (hb && d.hh_cap < hb) {
            d.hh_free();
            bool ok = false;
            on_node(d, [&] { ok = hipSetDevice(d.device) == hipSuccess && d.hh_alloc(hb); });
            if (!ok) return SID_ENOMEM;
        }
    }
    return SID_OK;
}

static int setup_generator(sid_engine* e)
{
    const size_t D = e->devs.size();
    if (e->src == SRC_SYNTH_HOST && e->gen_buf.size() != D) {
        e->gen_buf.assign(D, nullptr);
        e->gen_cap.assign(D, 0);
        e->gen_ev.assign(D, nullptr);
        for (size_t i = 0; i < D; ++i) {
            if (hipSetDevice(e->devs[i]->device) != hipSuccess) return SID_EHIP;
            if (hipEventCreateWithFlags(&e->gen_ev[i], hipEventDisableTiming) != hipSuccess) return SID_EHIP;
            if (hipEventRecord(e->gen_ev[i], e->devs[i]->s_up) != hipSuccess) return SID_EHIP;
        }
    }
    return SID_OK;
}

// The emit's pinned ring per device: 4 x 16 MiB (pinned once, reused by
// every run; 8 x 16, 4 x 64, 4 x 128 and 16 x 8 MiB measured slower: the
// pinning slows the ingest beside it and the exit tail grows with it)
constexpr int EMIT_RING_N = 4;
constexpr uint64_t EMIT_RING_BYTES = 16ull << 20;
static int alloc_ring_here(Dev& d);
// (on a thread bound to the GPU's CPUs: the ring's pages from its NUMA node)
static int alloc_ring(Dev& d)
{
    int rc = SID_OK;
    on_node(d, [&] { rc = alloc_ring_here(d); });
    return rc;
}
static int alloc_ring_here(Dev& d)
{
    if (hipSetDevice(d.device) != hipSuccess) return SID_EHIP;
    const uint64_t bytes = EMIT_RING_BYTES;
    while ((int)d.pinned.size() < EMIT_RING_N) {
        char* p = nullptr;
        hipEvent_t ev;
        if (hipHostMalloc((void**)&p, bytes, hipHostMallocDefault) != hipSuccess) return SID_ENOMEM;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
            (void)hipHostFree(p);
            return SID_EHIP;
        }
        d.pinned.push_back(p);
        d.pinned_ev.push_back(ev);
    }
    d.pinned_cap = bytes;
    return SID_OK;
}

// This run's strip crews (sid_engine_cfg.strip), one per pipeline, or none: the staging rings (made
// once, grown when a run's chunks are larger; on the GPU's NUMA node) and every job's regions.  Without
// the pinned memory for a ring the run goes without crews.
static void setup_strip(sid_engine* e, const std::vector<std::vector<uint64_t>>& lists)
{
    e->strip_runs.clear();
    if (!strip_eligible(e)) return;
    const int T = e->strip_T;
    for (size_t i = 0; i < e->devs.size(); ++i) {
        Dev& d = *e->devs[i];
        uint64_t need = 0;
        for (uint64_t j : lists[i]) need = std::max(need, e->recs[j].len);
        need += 64 * (uint64_t)(T + 2);
        bool ok = true;
        if (d.scap < need) on_node(d, [&] {
            ok = hipSetDevice(d.device) == hipSuccess;
            for (int b = 0; b < Dev::STRIP_RING && ok; ++b) {
                if (d.sbuf[b]) (void)hipHostFree(d.sbuf[b]);
                d.sbuf[b] = nullptr;
                d.scap = 0;
                ok = hipHostMalloc((void**)&d.sbuf[b], need, hipHostMallocDefault) == hipSuccess;
                if (ok && !d.sev[b]) ok = hipEventCreateWithFlags(&d.sev[b], hipEventDisableTiming) == hipSuccess;
            }
            if (ok) d.scap = need;
            else (void)hipGetLastError();
        });
        if (!ok) {
            e->strip_runs.clear();
            return;
        }
        auto S = std::make_unique<StripRun>();
        S->T = T;
        S->mode = e->cfg.strip;
        S->jobs.resize(lists[i].size());
        S->fin.assign(lists[i].size(), 0);
        for (size_t k = 0; k < lists[i].size(); ++k) {
            const ChunkRec& r = e->recs[lists[i][k]];
            StripJob& J = S->jobs[k];
            J.P.reset(new StripProg[T]);
            J.cut.assign(T + 1, r.len);
            J.cut[0] = 0;
            for (int t = 1; t < T; ++t) J.cut[t] = next_line_start(e->text + r.off, r.len, r.len * t / T);
        }
        e->strip_runs.push_back(std::move(S));
    }
}

// A parse error's offset in a chunk as the device saw it -> in the chunk's input bytes (ChunkRec::smap)
static uint64_t strip_unmap(const sid_engine* e, const ChunkRec& r, uint64_t off)
{
    uint64_t dev = 0, raw = 0;
    for (const auto& g : r.smap) {
        if (off < dev + g.dev)
            return raw + (g.stripped ? sid_strip_map(e->text + r.off + raw, g.raw, off - dev) : off - dev);
        dev += g.dev;
        raw += g.raw;
    }
    return raw + (off - dev);
}

extern "C" int sid_engine_ingest(sid_engine* e, sid_run_stats* st)
{
    if (!e || e->src == SRC_NONE) return SID_EINVAL;
    const double t0 = wall();
    reset_run(e);
    int rc = setup_budgets(e);
    const double t_budget = wall();
    if (rc == SID_OK) rc = setup_generator(e);
    if (rc != SID_OK) return rc;
    start_queues(e);
    const double t_setup = wall();
    const int D = (int)e->devs.size();
    // SID_ENGINE_TIMING: the first device's GPU timeline of the run -- its
    // start, and after the join the ends of its compute and D2H streams,
    // against its upload span (the head before the first copy, the tail
    // after the last)
    const bool timing = std::getenv("SID_ENGINE_TIMING") != nullptr;
    hipEvent_t tz[3] = {nullptr, nullptr, nullptr};
    if (timing) {
        Dev& d0 = *e->devs[0];
        for (auto& ev : tz) ev = d0.h2d_event();
        if (tz[0]) (void)hipEventRecord(tz[0], d0.s_up);
    }
    if (e->lynch)
        for (auto& dp : e->devs)
            if ((rc = sid_profile_reset(dp->ctx, dp->s_comp)) != SID_OK) return rc;
    std::vector<std::vector<uint64_t>> lists(D);
    for (uint64_t j = 0; j < e->recs.size(); ++j) lists[e->recs[j].dev].push_back(j);
    std::vector<std::function<void()>> th;
    setup_strip(e, lists);
    for (int i = 0; i < D; ++i) {
        Dev& d = *e->devs[i];
        const std::vector<uint64_t>& li = lists[i];
        StripRun* S = e->strip_runs.empty() ? nullptr : e->strip_runs[i].get();
        th.emplace_back([e, &d, &li, S] { uploader(e, d, li, 1, S); });
        th.emplace_back([e, &d] { compute(e, d, 1); });
        for (int t = 0; S && t < S->T; ++t) th.emplace_back([e, &d, &li, S, t] { strip_worker(e, d, *S, li, t); });
    }
    // the emit's pinned ring, pinned on a thread of its own during the ingest
    // of a run that writes its records through it (no host arena, no device
    // sink); a failure here leaves the ring to the emit, which reports it
    if (e->cfg.device_sink == 0 && e->cfg.host_hold_bytes == 0)
        th.emplace_back([e] {
            for (auto& dp : e->devs) (void)alloc_ring(*dp);
        });
    const double t_spawn = wall();
    e->crew.run(th);
    const double t_join = wall();
    if (e->rc.load() != SID_OK) {
        close_all(e);
        for (auto& dp : e->devs) (void)hipSetDevice(dp->device), (void)hipDeviceSynchronize();
        return e->rc.load();
    }
    if (timing) {
        Dev& d0 = *e->devs[0];
        if (tz[1]) (void)hipEventRecord(tz[1], d0.s_comp);
        if (tz[2]) (void)hipEventRecord(tz[2], d0.s_d2h);
        (void)hipSetDevice(d0.device);
        float head = -1.f, tc = -1.f, td = -1.f;
        if (hipStreamSynchronize(d0.s_comp) == hipSuccess && hipStreamSynchronize(d0.s_d2h) == hipSuccess &&
            hipStreamSynchronize(d0.s_up) == hipSuccess && !d0.h2d_pending.empty() && tz[0] && tz[1] && tz[2]) {
            (void)hipEventElapsedTime(&head, tz[0], d0.h2d_pending.front().first);
            (void)hipEventElapsedTime(&tc, d0.h2d_pending.back().second, tz[1]);
            (void)hipEventElapsedTime(&td, d0.h2d_pending.back().second, tz[2]);
        }
        (void)hipGetLastError();
        for (auto ev : tz)
            if (ev) d0.h2d_free.push_back(ev);
        std::fprintf(stderr,
                     "{\"ingest_setup_s\": %.6f, \"budgets_s\": %.6f, \"spawn_s\": %.6f, \"join_s\": %.6f, "
                     "\"gpu_head_ms\": %.3f, \"gpu_tail_comp_ms\": %.3f, \"gpu_tail_d2h_ms\": %.3f, \"join_after_ms\": %.3f}\n",
                     t_setup - t0, t_budget - t0, t_spawn - t_setup, t_join - t_spawn, head, tc, td,
                     (wall() - t_join) * 1e3);
    }
    double h2d_s = 0;
    uint64_t h2d_bytes = 0, tiled = 0, tile_over = 0, tile_oq = 0;
    for (auto& dp : e->devs) {
        (void)hipSetDevice(dp->device);
        if (hipStreamSynchronize(dp->s_comp) != hipSuccess || hipStreamSynchronize(dp->s_up) != hipSuccess ||
            hipStreamSynchronize(dp->s_d2h) != hipSuccess)
            return SID_EHIP;
        h2d_s += dp->h2d_collect();
        h2d_bytes += dp->h2d_bytes;
        dp->h2d_bytes = 0;
        tiled += dp->tiled;
        tile_over += dp->tile_overflows;
        tile_oq += dp->tile_over_queued;
        dp->tiled = dp->tile_overflows = dp->tile_over_queued = 0;
    }
    e->last_h2d_bytes = h2d_bytes;
    uint64_t sites = 0, bytes = 0, held = 0, kept = 0;
    for (auto& r : e->recs) {
        sites += r.parsed;
        bytes += src_bgzf(e->src) ? r.tlen : r.len;
        held += r.held != nullptr || r.host1 || r.sunk;
        kept += r.kept != nullptr;
    }
    if (st) {
        st->sites = sites;
        st->chunks = e->recs.size();
        st->bytes_in = e->src == SRC_SYNTH_HOST || e->src == SRC_SYNTH_DEVICE ? 0 : bytes;
        st->chunks_held = held;
        st->chunks_retained = kept;
        st->devices = D;
        st->status_kind = 0;
        st->err_offset = 0;
        st->ingest_s = wall() - t0;
        st->chunks_registered = e->reg_chunks.load();
        st->register_s = e->t_register.load() * 1e-9;
        st->h2d_s = h2d_s;
        st->h2d_bytes = h2d_bytes;
        st->chunks_tiled = tiled;
        st->tile_overflows = tile_over;
        st->tile_overflows_queued = tile_oq;
        st->bgzf_bytes = e->z_bytes.load();
        st->bgzf_blocks = e->z_blocks.load();
    }
    timing_report(e, "ingest", wall() - t0);
    const uint64_t fe = e->first_err.load();
    if (fe != UINT64_MAX) {
        const ChunkRec& r = e->recs[fe];
        if (r.zbad != ~0ull) {   // (a chunk with a bad member is not parsed: SID_EBGZF wins inside it)
            if (st) {
                st->status_kind = SID_EBGZF;
                st->err_offset = r.zbad;
            }
            return SID_EBGZF;
        }
        const unsigned kind = (unsigned)(r.err & 7);
        const int prc = kind == 1 ? SID_EMALFORMED : kind == 2 ? SID_ENULLCHROM : kind == 3 ? SID_EMISSING_MQ
                                                                                             : SID_ENOBQ;
        if (st) {
            st->status_kind = prc;
            st->err_offset = (src_bgzf(e->src) ? r.toff : r.off) + strip_unmap(e, r, r.err >> 3);
        }
        return prc;
    }
    e->ingested = true;
    e->estimated = !e->lynch;
    return SID_OK;
}

extern "C" int sid_engine_strip_stats(const sid_engine* e, uint64_t* chunks_stripped, uint64_t* strip_bytes)
{
    if (!e) return SID_EINVAL;
    if (chunks_stripped) *chunks_stripped = e->strip_chunks.load();
    if (strip_bytes) *strip_bytes = e->strip_bytes.load();
    return SID_OK;
}

// the pipelines' Lynch histograms merged (KB-sized tables) and loaded into
// every context, once per ingest (a second estimate, or a table loaded with
// sid_engine_profile_load, must not be merged again)
static int merge_histograms(sid_engine* e)
{
    const int D = (int)e->devs.size();
    if (D == 1 || e->hist_merged) {
        e->hist_merged = true;
        return SID_OK;
    }
    std::vector<std::vector<uint64_t>> k(D), v(D);
    std::vector<int> rcs(D, SID_OK);
    std::vector<std::thread> th;
    for (int i = 0; i < D; ++i)
        th.emplace_back([&, i] {
            size_t u = 0;
            sid_ctx* c = e->devs[i]->ctx;
            rcs[i] = sid_profile_table(c, nullptr, nullptr, 0, &u);
            if (rcs[i]) return;
            k[i].resize(u);
            v[i].resize(u);
            rcs[i] = sid_profile_table(c, k[i].data(), v[i].data(), u, &u);
        });
    for (auto& t : th) t.join();
    for (int r : rcs)
        if (r) return r;
    std::vector<uint64_t> K, V;
    for (int i = 0; i < D; ++i) {
        K.insert(K.end(), k[i].begin(), k[i].end());
        V.insert(V.end(), v[i].begin(), v[i].end());
    }
    for (int i = 0; i < D; ++i) {
        const int rc = sid_profile_load(e->devs[i]->ctx, K.data(), V.data(), K.size());
        if (rc != SID_OK) return rc;
    }
    e->hist_merged = true;
    return SID_OK;
}

extern "C" int sid_engine_profile_table(sid_engine* e, uint64_t* keys, uint64_t* counts64, size_t cap, size_t* u)
{
    if (!e || !u) return SID_EINVAL;
    if (!e->ingested || !e->lynch) return SID_ESTATE;
    const int rc = merge_histograms(e);
    if (rc != SID_OK) return rc;
    return sid_profile_table(e->devs[0]->ctx, keys, counts64, cap, u);
}

extern "C" int sid_engine_profile_load(sid_engine* e, const uint64_t* keys, const uint64_t* counts64, size_t u)
{
    if (!e || (!keys && u) || (!counts64 && u)) return SID_EINVAL;
    if (!e->ingested || !e->lynch) return SID_ESTATE;
    for (auto& dp : e->devs) {
        const int rc = sid_profile_load(dp->ctx, keys, counts64, u);
        if (rc != SID_OK) return rc;
    }
    e->hist_merged = true;
    return SID_OK;
}

extern "C" int sid_engine_records(sid_engine* e, uint64_t chunk, const char** bytes, uint64_t* len)
{
    if (!e || !bytes || !len || chunk >= e->recs.size()) return SID_EINVAL;
    const ChunkRec& r = e->recs[chunk];
    if (!r.host) return SID_ESTATE;
    *bytes = r.host;
    *len = r.host_len;
    return SID_OK;
}

extern "C" int sid_engine_estimate(sid_engine* e, const sid_estimate* given, sid_estimate* out)
{
    if (!e || !e->ingested) return SID_ESTATE;
    if (!e->lynch) {
        e->estimated = true;
        return SID_OK;
    }
    const int D = (int)e->devs.size();
    const int verbose = e->cfg.verbose;
    int rc = merge_histograms(e);
    if (rc != SID_OK) return rc;
    // one estimate (device 0, prints the reference's lines), the others
    // classify with its (pi, eps)
    sid_estimate est{};
    rc = sid_lynch_prepare_given(e->devs[0]->ctx, verbose, given, &est);
    if (rc != SID_OK) return rc;
    if (D > 1) {
        std::vector<int> rcs(D, SID_OK);
        std::vector<std::thread> th;
        for (int i = 1; i < D; ++i)
            th.emplace_back([&, i] { rcs[i] = sid_lynch_prepare_given(e->devs[i]->ctx, 0, &est, nullptr); });
        for (auto& t : th) t.join();
        for (int r : rcs)
            if (r) return r;
    }
    const int m = e->opts.method;
    if (m == SID_METHOD_LOCAL || m == SID_METHOD_QUALITY)   // -R: call.cpp:223-234, :305
        for (auto& dp : e->devs)
            if ((rc = sid_set_prior(dp->ctx, est.heterozygosity)) != SID_OK) return rc;
    e->est = est;
    if (out) *out = est;
    e->estimated = true;
    return SID_OK;
}

static int emit_records(sid_engine* e, const char* header, sid_write_fn write, void* user, sid_run_stats* st);

// the records, then (sid_opts.window) the chunks' rows stitched in file order
extern "C" int sid_engine_emit(sid_engine* e, const char* header, sid_write_fn write, void* user,
                               sid_run_stats* st)
{
    const int rc = emit_records(e, header, write, user, st);
    if (e && e->opts.window > 0 && rc != SID_ESTATE && rc != SID_EINVAL) {
        e->win.clear();
        e->win_ready = rc == SID_OK;
        if (rc == SID_OK) {
            e->win.window = e->opts.window;
            for (const auto& r : e->recs) sid_win_stitch_push(&e->win, r.win);
            e->win.finish();
        }
        if (st) st->window_rows = e->win.rows.size();
    }
    // ... and (sid_engine_set_depth_hist) the chunks' depth rows summed: a sorted merge per chunk
    if (e && e->depth_hist && rc != SID_ESTATE && rc != SID_EINVAL) {
        e->dh.clear();
        e->dh_ready = rc == SID_OK;
        if (rc == SID_OK)
            for (const auto& r : e->recs) sid_dh_add(&e->dh, r.dh);
    }
    // ... and (sid_engine_set_region_stats) the chunks' region rows summed into one entry per interval
    if (e && e->region_stats && rc != SID_ESTATE && rc != SID_EINVAL) {
        sid_region_stats_free(e->rs);
        e->rs = nullptr, e->rs_n = 0;
        e->rs_ready = false;
        const sid_regions* rg = e->devs[0]->ctx->regions_host;
        if (rc == SID_OK && rg) {
            std::vector<sid_rs_sum> tab(rg->start.size());
            for (const auto& r : e->recs) sid_rs_add(&tab, r.rs);
            const int xrc = sid_rs_export(rg, tab, false, &e->rs, &e->rs_n);
            if (xrc != SID_OK) return xrc;
            e->rs_ready = true;
        }
    }
    return rc;
}

extern "C" int sid_engine_set_depth_hist(sid_engine* e, int on)
{
    if (!e || (on != 0 && on != 1)) return SID_EINVAL;
    if (e->ingested) return SID_ESTATE;
    for (auto& d : e->devs) {
        // (a selection by label: through the context's route, whose parse keeps every site's label; the
        // region rows need the same route)
        const int rc = sid_ctx_label_route(d->ctx, on != 0 || e->region_stats);
        if (rc != SID_OK) return rc;
        sid_chunk_bind_context(&d->ws, d->ctx);
        d->ws.dh_on = on != 0;   // (the workspace's buffers: at its next reservation)
    }
    e->cx_n = e->devs[0]->ctx->cx_n;
    e->cx_on = e->devs[0]->ctx->cx_on;
    e->depth_hist = on != 0;
    e->dh.clear();
    e->dh_ready = false;
    return SID_OK;
}

extern "C" int sid_engine_set_region_stats(sid_engine* e, int on)
{
    if (!e || (on != 0 && on != 1)) return SID_EINVAL;
    const sid_regions* rg = e->devs[0]->ctx->regions_host;
    if (on && (!rg || sid_region_stats_valid(rg) != SID_OK)) return SID_EINVAL;
    if (e->ingested) return SID_ESTATE;
    for (auto& d : e->devs) {
        // (a selection by label: through the context's route, as the depth histogram)
        const int rc = sid_ctx_label_route(d->ctx, on != 0 || e->depth_hist);
        if (rc != SID_OK) return rc;
        sid_chunk_bind_context(&d->ws, d->ctx);
        d->ws.rs_on = on != 0;   // (the workspace's buffers: at its next reservation)
    }
    e->cx_n = e->devs[0]->ctx->cx_n;
    e->cx_on = e->devs[0]->ctx->cx_on;
    e->region_stats = on != 0;
    sid_region_stats_free(e->rs);
    e->rs = nullptr, e->rs_n = 0;
    e->rs_ready = false;
    return SID_OK;
}

extern "C" int sid_engine_region_stats(sid_engine* e, const sid_region_row** rows, size_t* n)
{
    if (!e || !rows || !n) return SID_EINVAL;
    *rows = nullptr, *n = 0;
    if (!e->region_stats || !e->rs_ready) return SID_ESTATE;
    *rows = e->rs;
    *n = e->rs_n;
    return SID_OK;
}

extern "C" int sid_engine_depth_hist(sid_engine* e, const sid_depth_row** rows, size_t* n)
{
    if (!e || !rows || !n) return SID_EINVAL;
    *rows = nullptr, *n = 0;
    if (!e->depth_hist || !e->dh_ready) return SID_ESTATE;
    *rows = e->dh.data();
    *n = e->dh.size();
    return SID_OK;
}

extern "C" int sid_engine_windows(sid_engine* e, const sid_window** rows, size_t* n)
{
    if (!e || !rows || !n) return SID_EINVAL;
    *rows = nullptr, *n = 0;
    if (e->opts.window <= 0 || !e->win_ready) return SID_ESTATE;
    *rows = e->win.rows.data();
    *n = e->win.rows.size();
    return SID_OK;
}

static int emit_records(sid_engine* e, const char* header, sid_write_fn write, void* user, sid_run_stats* st)
{
    if (!e || !e->ingested || !e->estimated) return SID_ESTATE;
    const int sink = e->cfg.device_sink;   // 0 write, 1 HBM only, 2 D2H only
    if (sink == 0 && !write) return SID_EINVAL;
    const double t0 = wall();
    e->rc = SID_OK;
    e->reloaded = 0;
    e->sink_bytes = 0;
    for (const auto& r : e->recs)
        if (r.sunk) e->sink_bytes += r.held_len;   // formatted and dropped in pass 1
    // every chunk's records already in the host arena (-m local / quality
    // with host_hold_bytes): nothing left for the devices, only the writes
    bool all_host = sink != 1;
    for (const auto& r : e->recs) all_host = all_host && r.host1;
    if (all_host) {
        uint64_t out = 0;
        bool ok = !(sink == 0 && header && write(user, header, std::strlen(header)) != 0);
        if (e->cx_on) {   // the forced edge records decided, and cut out
            if (sink == 0) {
                CxWriter cw(e, write, user);
                cw.ok = ok;
                for (uint64_t j = 0; j < e->recs.size(); ++j) {
                    cw.begin(j);
                    cw.piece(j, e->recs[j].host, e->recs[j].host_len);
                }
                cw.finish();
                ok = cw.ok;
            }
            out = cx_settle(e);
        } else {
            for (const auto& r : e->recs) {
                if (ok && sink == 0 && r.host_len && write(user, r.host, r.host_len) != 0) ok = false;
                out += r.host_len;
            }
        }
        if (st) {
            st->chunks_reloaded = 0;
            st->bytes_out = out;
            st->emit_s = wall() - t0;
        }
        timing_report(e, "emit", wall() - t0);
        e->ingested = false;
        return ok ? SID_OK : SID_EIO;
    }
    // the device sink with every chunk's records held in HBM since pass 1: no
    // pass 2 for the devices (the ingest synchronised their streams), only the
    // byte count -- no threads to start for a run that has nothing left to do
    bool all_held = sink == 1 && !e->recs.empty();
    for (const auto& r : e->recs) all_held = all_held && (r.held || r.sunk);
    if (all_held) {
        uint64_t out = 0;
        for (auto& r : e->recs) {
            Dev& d = *e->devs[r.dev];
            out += r.held_len;
            if (r.held) d.pool.put(r.held, r.held_cap, nullptr);
            if (r.kept) d.pool.put(r.kept, r.kept_cap, nullptr);
            if (r.pre) d.pool.put(r.pre, r.pre_cap, nullptr);
            r.held = r.kept = r.pre = nullptr;
        }
        if (e->cx_on) out = cx_settle(e);
        e->sink_bytes = out;
        if (st) {
            st->chunks_reloaded = 0;
            st->bytes_out = out;
            st->emit_s = wall() - t0;
        }
        timing_report(e, "emit", wall() - t0);
        e->ingested = false;
        return SID_OK;
    }
    start_queues(e);
    const int D = (int)e->devs.size();
    if (sink != 1)
        for (auto& dp : e->devs) {
            Dev& d = *dp;
            const int rc = alloc_ring(d);
            if (rc != SID_OK) return rc;
            for (int i = 0; i < EMIT_RING_N; ++i) d.free_pinned.push(i);
        }
    std::vector<std::vector<uint64_t>> lists(D);
    for (uint64_t j = 0; j < e->recs.size(); ++j) lists[e->recs[j].dev].push_back(j);
    std::atomic<uint64_t> out_bytes{0};
    std::vector<std::function<void()>> th;
    for (int i = 0; i < D; ++i) {
        Dev& d = *e->devs[i];
        const std::vector<uint64_t>& li = lists[i];
        th.emplace_back([e, &d, &li] { uploader(e, d, li, 2); });
        th.emplace_back([e, &d] { compute(e, d, 2); });
        if (sink != 1) th.emplace_back([e, &d] { drain(e, d); });
    }
    e->crew.start(th);
    // the writer: header, then every chunk's pieces in file order
    if (sink != 1) {
        bool ok = true;
        if (sink == 0 && header && write(user, header, std::strlen(header)) != 0) ok = false;
        // a context: the pieces go through the stitch (cxw; a chunk's descriptor is there before its first
        // piece: the compute thread read it back before it queued the chunk)
        std::unique_ptr<CxWriter> cxw;
        if (e->cx_on && sink == 0) cxw.reset(new CxWriter(e, write, user));
        bool cx_begun = false;
        auto emit_bytes = [&](uint64_t j, const char* p, uint64_t len) {
            if (!cxw) return !(sink == 0 && len && write(user, p, len) != 0);
            if (!cx_begun) cxw->begin(j), cx_begun = true;
            cxw->piece(j, p, len);
            return cxw->ok;
        };
        for (uint64_t j = 0; j < e->recs.size() && e->rc.load() == SID_OK; ++j) {
            Dev& d = *e->devs[e->recs[j].dev];
            const ChunkRec& rj = e->recs[j];
            cx_begun = false;
            if (rj.host1) {   // copied back during the ingest (which waited for the copies)
                if (ok && !emit_bytes(j, rj.host, rj.host_len)) ok = false;
                out_bytes += rj.host_len;
                if (!ok) break;
                continue;
            }
            Piece p;
            bool got_last = false;
            while (d.out_q.pop(p)) {
                if (p.host) {
                    const double w0 = wall();
                    const hipError_t ws = hipEventSynchronize(p.hev);
                    e->t_write_wait += (uint64_t)((wall() - w0) * 1e9);
                    d.give_event(p.hev);
                    if (ws != hipSuccess) {
                        fail(e, SID_EHIP);
                        break;
                    }
                    if (ok && !emit_bytes(j, p.host, p.len)) ok = false;
                    out_bytes += p.len;
                } else if (p.ps >= 0) {
                    const double w0 = wall();
                    const hipError_t ws = hipEventSynchronize(d.pinned_ev[p.ps]);
                    e->t_write_wait += (uint64_t)((wall() - w0) * 1e9);
                    if (ws != hipSuccess) {
                        fail(e, SID_EHIP);
                        break;
                    }
                    if (ok && !emit_bytes(j, d.pinned[p.ps], p.len)) ok = false;
                    out_bytes += p.len;
                    d.free_pinned.push(p.ps);
                }
                if (p.last) {
                    d.pool.put(p.buf, p.cap, nullptr);   // its D2H completed (event above)
                    got_last = true;
                    if (cxw && !cx_begun) cxw->begin(j);   // (a chunk without bytes: its descriptor all the same)
                    break;
                }
            }
            if (!ok) fail(e, SID_EIO);
            if (!got_last) break;
        }
        if (cxw && ok && e->rc.load() == SID_OK) {
            cxw->finish();
            ok = cxw->ok;
        }
        if (!ok) fail(e, SID_EIO);
        if (e->rc.load() != SID_OK) close_all(e);
    }
    e->crew.wait();
    for (auto& dp : e->devs) {
        (void)hipSetDevice(dp->device);
        if (hipDeviceSynchronize() != hipSuccess) fail(e, SID_EHIP);
    }
    const bool cx_done = e->cx_on && e->rc.load() == SID_OK;
    const uint64_t cx_out = cx_done ? cx_settle(e) : 0;
    if (st) {
        st->chunks_reloaded = e->reloaded.load();
        st->bytes_out = sink == 1 ? e->sink_bytes.load() : out_bytes.load();
        if (cx_done) st->bytes_out = cx_out;
        st->emit_s = wall() - t0;
    }
    timing_report(e, "emit", wall() - t0);
    // every held / kept buffer went back to the pools
    for (auto& r : e->recs) {
        Dev& d = *e->devs[r.dev];
        if (r.held) d.pool.put(r.held, r.held_cap, nullptr);
        if (r.kept) d.pool.put(r.kept, r.kept_cap, nullptr);
        if (r.pre) d.pool.put(r.pre, r.pre_cap, nullptr);
        r.held = r.kept = r.pre = nullptr;
    }
    e->ingested = false;
    return e->rc.load();
}

extern "C" int sid_engine_run(sid_engine* e, const char* header, sid_write_fn write, void* user,
                              sid_run_stats* st)
{
    if (!e) return SID_EINVAL;
    sid_run_stats local{};
    sid_run_stats* s = st ? st : &local;
    std::memset(s, 0, sizeof *s);
    int rc = sid_engine_ingest(e, s);
    if (rc != SID_OK) return rc;
    const double t0 = wall();
    rc = sid_engine_estimate(e, nullptr, &s->estimate);
    s->estimate_s = wall() - t0;
    if (rc != SID_OK) return rc;
    return sid_engine_emit(e, header, write, user, s);
}

extern "C" int sid_engine_profile(sid_engine* e, int enable)
{
    if (!e) return SID_EINVAL;
    e->prof = enable != 0;
    return SID_OK;
}

// sums the pending event pairs of every device (after their streams drained)
extern "C" int sid_engine_profile_read(sid_engine* e, sid_engine_prof* out)
{
    if (!e || !out) return SID_EINVAL;
    for (auto& dp : e->devs) {
        Dev& d = *dp;
        if (hipSetDevice(d.device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return SID_EHIP;
        for (auto& pr : d.prof_pending) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, pr.second.first, pr.second.second) == hipSuccess) e->prof_ms[pr.first] += ms;
            d.prof_free.push_back(pr.second.first);
            d.prof_free.push_back(pr.second.second);
        }
        d.prof_pending.clear();
        e->prof_chunks += d.prof_chunks;
        d.prof_chunks = 0;
    }
    std::memset(out, 0, sizeof *out);
    out->chunks = e->prof_chunks;
    out->index_ms = e->prof_ms[0];
    out->parse_ms = e->prof_ms[1];
    out->call_ms = e->prof_ms[2];
    out->hist_ms = e->prof_ms[3];
    out->fmt_len_ms = e->prof_ms[4];
    out->fmt_write_ms = e->prof_ms[5];
    for (double& v : e->prof_ms) v = 0;
    e->prof_chunks = 0;
    return SID_OK;
}
