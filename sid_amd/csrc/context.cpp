// context.cpp — the context on the host (context.h): sid_context_mark for
// records formatted on the host, and the stitch of the chunks' forced edge
// records for the engine's emit.  Pure host code, no HIP call.
#include "context.h"

#include <algorithm>
#include <cstring>

// --context on the host path: a forward and a backward walk over the records
// of U (the sites code_all does not drop), each carrying the records since /
// until the nearest selected one (the sites `code` still keeps), saturated
extern "C" int sid_context_mark(const uint8_t* code_all, uint8_t* code, size_t n, int context)
{
    if (context < 0 || context > SID_CONTEXT_MAX) return SID_EINVAL;
    if (n && (!code_all || !code)) return SID_EINVAL;
    if (context == 0) return SID_OK;
    const uint32_t N = (uint32_t)context;
    std::vector<uint8_t> near(n, 0);
    uint32_t d = N + 1;   // records since the last selected one
    for (size_t i = 0; i < n; ++i) {
        if (code_all[i] & SID_CODE_DROPPED) continue;
        if (!(code[i] & SID_CODE_DROPPED)) d = 0;
        else if (d <= N) ++d;
        if (d <= N) near[i] = 1;
    }
    d = N + 1;
    for (size_t i = n; i-- > 0;) {
        if (code_all[i] & SID_CODE_DROPPED) continue;
        if (!(code[i] & SID_CODE_DROPPED)) d = 0;
        else if (d <= N) ++d;
        if (d <= N || near[i]) code[i] &= (uint8_t)~SID_CODE_DROPPED;
    }
    return SID_OK;
}

void sid_cx_stitch::keep_bit(sid_cx_verdict& v, uint32_t records, uint32_t idx)
{
    const uint32_t z = std::min(records, n_);
    if (idx < z) v.head_keep |= 1ull << idx;
    if (idx >= records - z) v.tail_keep |= 1ull << (idx - (records - z));
}

void sid_cx_stitch::settle()
{
    resolved_ = pend_.empty() ? v_.size() : pend_.front().chunk;
}

void sid_cx_stitch::push(const sid_cx_desc& d)
{
    const uint32_t R = d.records, z = std::min(R, n_);
    // the chunks whose last records waited for a selected record behind them
    size_t w = 0;
    for (size_t k = 0; k < pend_.size(); ++k) {
        Pending p = pend_[k];
        if (d.has_sel) {   // the nearest one behind: d.lead records into this chunk
            for (uint32_t idx = p.first; idx < p.records; ++idx)
                if ((uint64_t)(p.records - 1 - idx) + p.after + d.lead + 1 <= n_) keep_bit(v_[p.chunk], p.records, idx);
            continue;
        }
        p.after = (uint32_t)std::min<uint64_t>((uint64_t)p.after + R, n_ + 1);
        if (p.after >= n_) continue;   // out of every later record's reach
        pend_[w++] = p;
    }
    pend_.resize(w);
    // this chunk: the in-chunk verdicts (a record in both zones: either's), then
    // the reach of the last selected record in front of the chunk
    sid_cx_verdict v;
    const uint64_t zm = z == 64 ? ~0ull : (1ull << z) - 1;
    for (uint32_t k = 0; k < z; ++k) {
        if ((d.head_keep & zm) >> k & 1) keep_bit(v, R, k);
        if ((d.tail_keep & zm) >> k & 1) keep_bit(v, R, R - z + k);
    }
    for (uint32_t idx = 0; idx < z && since_ + idx + 1 <= n_; ++idx) keep_bit(v, R, idx);
    const size_t c = v_.size();
    v_.push_back(v);
    // its records behind its last selected one that a later chunk may reach
    const uint32_t tr = d.has_sel ? std::min(d.trail, R) : R;
    const uint32_t first = std::max(R - z, R - tr);
    if (first < R) pend_.push_back(Pending{c, first, 0, R});
    since_ = d.has_sel ? std::min(d.trail, n_ + 1) : (uint32_t)std::min<uint64_t>((uint64_t)since_ + R, n_ + 1);
    settle();
}

void sid_cx_stitch::finish()
{
    pend_.clear();
    settle();
}

size_t sid_cx_ranges(const sid_cx_desc& d, int context, const sid_cx_verdict& v, uint64_t total, sid_cx_range* out,
                     uint64_t* kept)
{
    const uint32_t R = d.records, z = sid_cx_zone(d, context);
    size_t nr = 0;
    uint64_t sum = 0;
    auto add = [&](uint64_t off, uint64_t len) {
        if (!len) return;
        sum += len;
        if (nr && out[nr - 1].off + out[nr - 1].len == off) out[nr - 1].len += len;
        else out[nr++] = sid_cx_range{off, len};
    };
    uint64_t head = 0, tail = 0;
    for (uint32_t k = 0; k < z; ++k) head += d.head_len[k], tail += d.tail_len[k];
    if (z == 0 || head > total || tail > total) {   // (no forced record; or lengths that are not this chunk's: all of it)
        add(0, total);
        if (kept) *kept = sum;
        return nr;
    }
    uint64_t at = 0;
    for (uint32_t k = 0; k < z; ++k) {
        if (v.head_keep >> k & 1) add(at, d.head_len[k]);
        at += d.head_len[k];
    }
    const uint64_t t0 = total - tail;
    if (t0 > at) add(at, t0 - at);   // between the zones: decided on the device
    at = t0;
    for (uint32_t k = 0; k < z; ++k) {
        const uint32_t idx = R - z + k;
        if (idx >= z && (v.tail_keep >> k & 1)) add(at, d.tail_len[k]);   // (idx < z: the head zone's record)
        at += d.tail_len[k];
    }
    if (kept) *kept = sum;
    return nr;
}

uint64_t sid_cx_compact(char* bytes, const sid_cx_range* r, size_t nr)
{
    uint64_t at = 0;
    for (size_t k = 0; k < nr; ++k) {
        if (r[k].off != at) std::memmove(bytes + at, bytes + r[k].off, r[k].len);
        at += r[k].len;
    }
    return at;
}

extern "C" void sid_cx_edge_lengths(const char* bytes, uint64_t total, int context, sid_cx_desc* d)
{
    const uint32_t z = sid_cx_zone(*d, context);
    std::memset(d->head_len, 0, sizeof d->head_len);
    std::memset(d->tail_len, 0, sizeof d->tail_len);
    uint64_t at = 0;
    for (uint32_t k = 0; k < z && at < total; ++k) {
        const void* nl = std::memchr(bytes + at, '\n', total - at);
        const uint64_t end = nl ? (uint64_t)((const char*)nl - bytes) + 1 : total;
        d->head_len[k] = (uint32_t)(end - at);
        at = end;
    }
    uint64_t end = total;
    for (uint32_t k = z; k-- > 0 && end > 0;) {
        uint64_t b = end - 1;   // (the record's own newline, or its last byte when the chunk's end lacks one)
        while (b > 0 && bytes[b - 1] != '\n') --b;
        d->tail_len[k] = (uint32_t)(end - b);
        end = b;
    }
}

extern "C" int sid_cx_stitch_chunks(const sid_cx_desc* d, size_t n, int context, char* bytes, const uint64_t* off,
                                    uint64_t* len)
{
    if (context < 0 || context > SID_CONTEXT_MAX) return SID_EINVAL;
    if (n && (!d || !off || !len)) return SID_EINVAL;
    sid_cx_stitch S(context);
    for (size_t c = 0; c < n; ++c) S.push(d[c]);
    S.finish();
    sid_cx_range g[2 * SID_CONTEXT_MAX + 1];
    for (size_t c = 0; c < n; ++c) {
        const size_t nr = sid_cx_ranges(d[c], context, S.verdict(c), len[c], g, nullptr);
        len[c] = sid_cx_compact(bytes + off[c], g, nr);
    }
    return SID_OK;
}
