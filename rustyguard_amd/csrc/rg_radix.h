// rg_radix.h -- stable grouping of a batch's packet indices by a 32-bit key: the passes of an LSD radix
// sort, 8 bits per pass, shared by the device anti-replay commit (rg_replay.hip: key = window row) and the
// device send-counter reservation (rg_send.hip: key = session row).  Device code only.
//
// KeyOf is a small struct passed by value with `__device__ uint32_t operator()(uint32_t i) const`: the
// grouping key of packet i.  One pass:
//   radix_hist_kernel     digit counts per workgroup of kRadixTile positions
//   radix_scan_kernel     exclusive prefix sum over the digit-major counts, one workgroup
//   radix_scatter_kernel  stable scatter behind those offsets
// group_by_key runs as many passes as the key range needs and returns the grouped order (nullptr for no
// pass: the array is its own grouping).
#pragma once
#include "rg_internal.h"

namespace rg {

constexpr uint32_t kRadixTile = kReplayTile; // positions per workgroup of 256 lanes
constexpr uint32_t kRadixItems = kRadixTile / 256;

// 8-bit passes that order keys below nkeys (0: one key, no grouping)
__host__ __device__ inline uint32_t radix_passes(uint32_t nkeys) {
    uint32_t p = 0;
    for (uint32_t top = nkeys ? nkeys - 1 : 0; top; top >>= 8) ++p;
    return p;
}

// One pass of a stable LSD radix sort: workgroup b owns positions [b, b + 1) x kRadixTile of src
// (src == nullptr: the identity).
template <class KeyOf>
__global__ __launch_bounds__(256) void radix_hist_kernel(KeyOf key, uint32_t n, uint32_t nblk, const uint32_t *src,
                                                         uint32_t shift, uint32_t *hist) {
    __shared__ uint32_t s_h[256];
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kRadixTile;
    for (uint32_t k = 0; k < kRadixItems; ++k) {
        const uint64_t pos = base + k * 256 + threadIdx.x;
        if (pos < n) atomicAdd(&s_h[(key(src ? src[pos] : (uint32_t)pos) >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(uint64_t)threadIdx.x * nblk + blockIdx.x] = s_h[threadIdx.x];
}

// exclusive prefix sum over hist[0, total), digit-major: one workgroup, a contiguous run per lane (a
// template like its neighbours, so that each file that groups owns its instance)
template <class KeyOf>
__global__ __launch_bounds__(1024) void radix_scan_kernel(uint32_t *hist, uint64_t total) {
    __shared__ uint32_t s_sum[1024];
    const uint32_t t = threadIdx.x;
    const uint64_t per = (total + 1023) / 1024, lo = min(t * per, total), hi = min(lo + per, total);
    uint32_t sum = 0;
    for (uint64_t j = lo; j < hi; ++j) sum += hist[j];
    s_sum[t] = sum;
    __syncthreads();
    uint32_t cur = sum;
    for (uint32_t off = 1; off < 1024; off <<= 1) {
        const uint32_t o = t >= off ? s_sum[t - off] : 0u;
        __syncthreads();
        cur += o;
        s_sum[t] = cur;
        __syncthreads();
    }
    uint32_t run = cur - sum;
    for (uint64_t j = lo; j < hi; ++j) {
        const uint32_t c = hist[j];
        hist[j] = run;
        run += c;
    }
}

// Stable scatter: wave v of the workgroup owns the contiguous quarter v of the tile and walks it 64
// positions at a time; lanes of one round with the same digit find each other by ballots and take
// consecutive places behind the digit's running offset.
template <class KeyOf>
__global__ __launch_bounds__(256) void radix_scatter_kernel(KeyOf key, uint32_t n, uint32_t nblk, const uint32_t *src,
                                                            uint32_t *dst, uint32_t shift, const uint32_t *hist) {
    __shared__ uint32_t s_off[4][256];
    const uint32_t t = threadIdx.x, v = t >> 6, lane = t & 63;
    for (uint32_t q = 0; q < 4; ++q) s_off[q][t] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kRadixTile + v * (kRadixTile / 4);
    constexpr uint32_t kRounds = kRadixTile / 256;
    uint32_t idx[kRounds], dg[kRounds];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint64_t pos = base + r * 64 + lane;
        const bool ok = pos < n;
        idx[r] = ok ? (src ? src[pos] : (uint32_t)pos) : 0u;
        dg[r] = ok ? (key(idx[r]) >> shift) & 255u : 256u;
        if (ok) atomicAdd(&s_off[v][dg[r]], 1u);
    }
    __syncthreads();
    { // counts -> first place of (wave, digit): the workgroup's base, then the waves in order
        uint32_t run = hist[(uint64_t)t * nblk + blockIdx.x];
        for (uint32_t q = 0; q < 4; ++q) {
            const uint32_t c = s_off[q][t];
            s_off[q][t] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const bool ok = dg[r] < 256u;
        uint64_t same = __ballot(ok);
#pragma unroll
        for (uint32_t b = 0; b < 8; ++b) {
            const bool bit = (dg[r] >> b) & 1u;
            const uint64_t m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1));
        const uint32_t off = ok ? s_off[v][dg[r]] : 0u;
        __syncthreads();
        if (ok && rank == 0) s_off[v][dg[r]] = off + (uint32_t)__popcll(same);
        if (ok) dst[(uint64_t)off + rank] = idx[r];
        __syncthreads();
    }
}

// The grouped order of [0, n) under `key`: `passes` passes ping-ponging between order0 and order1 (order1
// is touched only from the second pass on), hist = [256][nblk] u32.  Returns where the last pass wrote, or
// nullptr when passes == 0.
template <class KeyOf>
inline const uint32_t *group_by_key(KeyOf key, uint32_t n, uint32_t nblk, uint32_t passes, uint32_t *hist,
                                    uint32_t *order0, uint32_t *order1, hipStream_t st) {
    const dim3 tiles(nblk), wg(256);
    const uint32_t *src = nullptr;
    for (uint32_t p = 0; p < passes; ++p) {
        uint32_t *dst = (p & 1) ? order1 : order0;
        hipLaunchKernelGGL(radix_hist_kernel<KeyOf>, tiles, wg, 0, st, key, n, nblk, src, 8 * p, hist);
        hipLaunchKernelGGL(radix_scan_kernel<KeyOf>, dim3(1), dim3(1024), 0, st, hist, 256ull * nblk);
        hipLaunchKernelGGL(radix_scatter_kernel<KeyOf>, tiles, wg, 0, st, key, n, nblk, src, dst, 8 * p,
                           (const uint32_t *)hist);
        src = dst;
    }
    return src;
}

} // namespace rg
