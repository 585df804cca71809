// inflate.hip — BGZF members inflated on the device: one wave64 per member,
// the decoder core of bgzf.h with a wave-wide output policy.
//
// The symbol loop is uniform over the wave (bit buffer, positions and table
// entries pass through readfirstlane, so they live in scalar registers); the
// Huffman tables of the current deflate block sit in LDS (4 KiB + the 1 KiB
// CRC table per wave, so LDS does not bound occupancy).  The lanes share what
// is parallel: a run of up to 64 literals is held one byte per lane and
// written by one store, a match is copied 64 bytes per step (source index
// pos - distance + (i mod distance) when the copy overlaps itself), stored
// bytes likewise.  Output goes straight to HBM and back-references are read
// back from it: a wave's stores and later loads go through the same L1 in
// order, the workgroup fence in front of each copy makes that explicit.  The
// CRC32 is taken by the lanes over 64 spans, each span's remainder shifted
// over the bytes behind it (square-and-multiply) and xor-reduced.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "bgzf_dev.h"
#include "sid_internal.h"

namespace {

struct wave_out {
    uint8_t* o;
    uint32_t pos, cap;
    uint32_t lane;
    uint32_t lb;   // this lane's byte of the pending literal run [ps, pos), pos - ps <= 64
    uint32_t ps;
    __device__ void flush()
    {
        if (pos != ps) {
            const uint32_t p = ps + ((lane - ps) & 63);   // the run's position that is this lane's (mod 64)
            if (p < pos) o[p] = (uint8_t)lb;
            ps = pos;
        }
    }
    __device__ void lit(uint8_t c)
    {
        if (lane == (pos & 63)) lb = c;
        ++pos;
        if (pos - ps == 64) flush();
    }
    __device__ void copy(uint32_t dist, uint32_t len)
    {
        flush();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the bytes behind pos, whichever lane stored them
        const uint8_t* src = o + pos - dist;
        if (dist >= len) {
            for (uint32_t i = lane; i < len; i += 64) o[pos + i] = src[i];
        } else {
            for (uint32_t i = lane; i < len; i += 64) o[pos + i] = src[i % dist];
        }
        pos += len;
        ps = pos;
    }
    __device__ void raw(const uint8_t* s, uint32_t len)
    {
        flush();
        for (uint32_t i = lane; i < len; i += 64) o[pos + i] = s[i];
        pos += len;
        ps = pos;
    }
    __device__ void finish()
    {
        flush();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the CRC's lanes read what other lanes stored
    }
};

__global__ __launch_bounds__(64) void bgzf_inflate_k(const uint8_t* __restrict__ in,
                                                      const sid_bgzf_dblk* __restrict__ tab, uint32_t nblocks,
                                                      uint8_t* out, uint32_t* __restrict__ status)
{
    __shared__ bgzf_tables T;
    __shared__ uint32_t crct[256];
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    if (k >= nblocks) return;
    for (uint32_t j = lane; j < 256; j += 64) crct[j] = bgzf_crc_entry(j);
    __syncthreads();
    const sid_bgzf_dblk blk = tab[k];
    const uint8_t* p = in + blk.coff;
    bgzf_member m;
    int rc = bgzf_member_parse(p, blk.csize, &m);
    if (rc == BGZF_OK && (m.bsize != blk.csize || m.isize != blk.isize)) rc = BGZF_EHEADER;
    if (rc == BGZF_OK) {
        wave_out o{out + blk.ooff, 0, blk.isize, lane, 0, 0};
        rc = bgzf_inflate(p + m.hdr, blk.csize - m.hdr - 8, o, T);
        if (rc == BGZF_OK) {
            uint32_t x = bgzf_crc_lane(crct, o.o, blk.isize, lane, 64);
            for (int off = 32; off > 0; off >>= 1) x ^= (uint32_t)__shfl_xor((int)x, off, 64);
            if (bgzf_crc_finish(0, x, blk.isize) != m.crc) rc = BGZF_ECRC;
        }
    }
    // (the lane number read afresh, not carried through the divergent CRC code above)
    if (__lane_id() == 0) status[k] = (uint32_t)rc;
}

// the status words reduced to the lowest member whose status is not BGZF_OK (0xffffffff: none)
__global__ __launch_bounds__(256) void bgzf_status_k(const uint32_t* __restrict__ status, uint32_t nblocks,
                                                      uint32_t* __restrict__ bad)
{
    __shared__ uint32_t wmin[4];
    uint32_t lo = 0xffffffffu;
    for (uint32_t k = threadIdx.x; k < nblocks; k += 256)
        if (status[k] != BGZF_OK) lo = min(lo, k);
    for (int off = 32; off > 0; off >>= 1) lo = min(lo, (uint32_t)__shfl_xor((int)lo, off, 64));
    if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = lo;
    __syncthreads();
    if (threadIdx.x == 0) *bad = min(min(wmin[0], wmin[1]), min(wmin[2], wmin[3]));
}

}   // namespace

hipError_t sid_launch_bgzf_inflate(const uint8_t* d_in, const sid_bgzf_dblk* d_tab, uint32_t nblocks, uint8_t* d_out,
                                   uint32_t* d_status, uint32_t* d_bad, hipStream_t st)
{
    if (nblocks)
        hipLaunchKernelGGL(bgzf_inflate_k, dim3(nblocks), dim3(64), 0, st, d_in, d_tab, nblocks, d_out, d_status);
    hipLaunchKernelGGL(bgzf_status_k, dim3(1), dim3(256), 0, st, d_status, nblocks, d_bad);
    return hipGetLastError();
}

extern "C" int sid_bgzf_inflate_device(sid_ctx* ctx, const void* d_bytes, const sid_bgzf* z, size_t first_block,
                                       size_t nblocks, char* d_out, size_t cap, uint64_t* err_block, void* stream)
{
    if (err_block) *err_block = 0;
    if (!ctx || !z || first_block > z->blk.size() || nblocks > z->blk.size() - first_block) return SID_EINVAL;
    if (nblocks == 0) return SID_OK;
    if (!d_bytes || !d_out || nblocks > 0xfffffffeu) return SID_EINVAL;
    const uint64_t t0 = z->blk[first_block].toff;
    const sid_bgzf_blk& lastb = z->blk[first_block + nblocks - 1];
    if (lastb.toff + lastb.isize - t0 > cap) return SID_ENOMEM;
    hipStream_t st = (hipStream_t)stream;
    // the kernel takes the members that hold text; an empty member (the EOF marker) is read back and
    // checked here, by the host build of the same decoder
    std::vector<sid_bgzf_dblk> h;
    std::vector<size_t> which;
    size_t bad_empty = SIZE_MAX;
    std::vector<uint8_t> tmp;
    for (size_t k = 0; k < nblocks; ++k) {
        const sid_bgzf_blk& b = z->blk[first_block + k];
        if (b.isize) {
            h.push_back(sid_bgzf_dblk{b.coff, (int64_t)(b.toff - t0), b.csize, b.isize});
            which.push_back(k);
        } else if (bad_empty == SIZE_MAX) {
            uint8_t none;
            tmp.resize(b.csize);
            // (pageable host memory on both sides of this call: blocking copies, ordered by hand
            // against the caller's stream)
            const hipError_t xs = hipStreamSynchronize(st);
            const hipError_t x = hipMemcpy(tmp.data(), (const char*)d_bytes + b.coff, b.csize, hipMemcpyDeviceToHost);
            if (x != hipSuccess || xs != hipSuccess) return sid_set_hip_error(x != hipSuccess ? x : xs);
            if (sid_bgzf_inflate_block(tmp.data(), b.csize, 0, &none) != BGZF_OK) bad_empty = k;
        }
    }
    nblocks = h.size();
    auto verdict = [&](size_t bad_dev) {
        const size_t bad = std::min(bad_dev, bad_empty);
        if (bad == SIZE_MAX) return (int)SID_OK;
        if (err_block) *err_block = first_block + bad;
        return (int)SID_EBGZF;
    };
    if (nblocks == 0) return verdict(SIZE_MAX);
    char* d = nullptr;
    const size_t tab_bytes = nblocks * sizeof(sid_bgzf_dblk), all = tab_bytes + (nblocks + 1) * sizeof(uint32_t);
    hipError_t e = hipMalloc((void**)&d, all);
    if (e != hipSuccess) return sid_set_hip_error(e);
    sid_bgzf_dblk* d_tab = (sid_bgzf_dblk*)d;
    uint32_t* d_status = (uint32_t*)(d + tab_bytes);
    uint32_t* d_bad = d_status + nblocks;
    uint32_t bad = 0xffffffffu;
    e = hipMemcpy(d_tab, h.data(), tab_bytes, hipMemcpyHostToDevice);   // (done when it returns)
    if (e == hipSuccess)
        e = sid_launch_bgzf_inflate((const uint8_t*)d_bytes, d_tab, (uint32_t)nblocks, (uint8_t*)d_out, d_status, d_bad,
                                    st);
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return sid_set_hip_error(e);
    return verdict(bad != 0xffffffffu ? which[bad] : SIZE_MAX);
}
