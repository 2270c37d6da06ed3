// Device scan and stable LSD radix sort shared by the device dataset build (cont_data_dev.hip) and the simulator
// (cont_simulate.hip): integer exclusive scans over tiles of DD_TILE elements, and a stable sort by 8-bit digits
// (digit histograms, digit-major scan, wave64 ballot ranks) with int32 payloads.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "nhp_internal.h"

#define DD_BLOCK 256                     // 4 waves
#define DD_ITEMS 8                       // elements per thread of a scan / sort tile
#define DD_TILE (DD_BLOCK * DD_ITEMS)
#define DD_RADIX 256                     // 8-bit digits (one LDS counter per thread of a block)

static inline unsigned dd_grid(int64_t n, int64_t per) { return (unsigned)std::max<int64_t>(1, (n + per - 1) / per); }
static inline int dd_bitlen(uint64_t v) { int b = 0; while (b < 64 && (v >> b) != 0) ++b; return b; }

// ---- primitives: exclusive scan and stable LSD radix sort ---------------------------------------------------------

// exclusive scan of v over the block (every thread calls it); *total = the block's sum
template <typename T>
__device__ T dd_block_exclusive(T v, T *wsum, T *total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    T off = 0, tot = 0;
    for (int q = 0; q < DD_BLOCK / 64; ++q) { if (q < w) off += wsum[q]; tot += wsum[q]; }
    __syncthreads();
    *total = tot;
    return off + x - v;
}

template <typename T>
__global__ void __launch_bounds__(DD_BLOCK) k_dd_tile_sum(const T *__restrict__ in, int64_t n, T *__restrict__ sums)
{
    __shared__ T wsum[DD_BLOCK / 64];
    const int64_t i0 = (int64_t)blockIdx.x * DD_TILE + (int64_t)threadIdx.x * DD_ITEMS;
    T s = 0;
    for (int r = 0; r < DD_ITEMS; ++r)
        if (i0 + r < n) s += in[i0 + r];
    T tot;
    (void)dd_block_exclusive(s, wsum, &tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// one workgroup: the tile sums in place, exclusive; the grand total to *total
template <typename T>
__global__ void __launch_bounds__(DD_BLOCK) k_dd_scan_sums(T *__restrict__ sums, int64_t nt, T *__restrict__ total)
{
    __shared__ T wsum[DD_BLOCK / 64];
    T carry = 0;
    for (int64_t j0 = 0; j0 < nt; j0 += DD_BLOCK) {
        const int64_t j = j0 + threadIdx.x;
        const T v = j < nt ? sums[j] : (T)0;
        T tot;
        const T ex = dd_block_exclusive(v, wsum, &tot);
        if (j < nt) sums[j] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

template <typename T>
__global__ void __launch_bounds__(DD_BLOCK) k_dd_tile_scan(const T *__restrict__ in, int64_t n, const T *__restrict__ sums,
                                                           T *__restrict__ out)
{
    __shared__ T wsum[DD_BLOCK / 64];
    const int64_t i0 = (int64_t)blockIdx.x * DD_TILE + (int64_t)threadIdx.x * DD_ITEMS;
    T v[DD_ITEMS], s = 0;
    for (int r = 0; r < DD_ITEMS; ++r) { v[r] = i0 + r < n ? in[i0 + r] : (T)0; s += v[r]; }
    T tot;
    T run = sums[blockIdx.x] + dd_block_exclusive(s, wsum, &tot);
    for (int r = 0; r < DD_ITEMS; ++r)
        if (i0 + r < n) { out[i0 + r] = run; run += v[r]; }
}

// out[0..n] = exclusive prefix sums of in[0..n), out[n] = the total; tmp holds ceil(n / DD_TILE) values
template <typename T>
static void dd_scan(hipStream_t st, const T *in, T *out, int64_t n, T *tmp)
{
    if (n == 0) { (void)hipMemsetAsync(out, 0, sizeof(T), st); return; }
    const unsigned nt = dd_grid(n, DD_TILE);
    k_dd_tile_sum<T><<<nt, DD_BLOCK, 0, st>>>(in, n, tmp);
    k_dd_scan_sums<T><<<1, DD_BLOCK, 0, st>>>(tmp, nt, out + n);
    k_dd_tile_scan<T><<<nt, DD_BLOCK, 0, st>>>(in, n, tmp, out);
}

// digit histogram of each tile, digit-major: hist[d * nt + tile]
template <typename K>
__global__ void __launch_bounds__(DD_BLOCK) k_dd_hist(const K *__restrict__ keys, int64_t n, int shift, uint32_t *__restrict__ hist,
                                                      unsigned nt)
{
    __shared__ uint32_t h[DD_RADIX];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t tile = (int64_t)blockIdx.x * DD_TILE;
    for (int r = 0; r < DD_ITEMS; ++r) {
        const int64_t k = tile + r * DD_BLOCK + threadIdx.x;
        if (k < n) atomicAdd(&h[(uint32_t)(keys[k] >> shift) & (DD_RADIX - 1)], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * nt + blockIdx.x] = h[threadIdx.x];
}

// Stable scatter of one tile: sub-rounds of DD_BLOCK elements in order; inside a wave the lanes holding the same digit
// are found with 8 ballots (64-bit masks), a lane's rank is the number of such lanes below it; waves in order after that.
// vin = nullptr: the values are the element indices.
template <typename K>
__global__ void __launch_bounds__(DD_BLOCK) k_dd_scatter(const K *__restrict__ kin, const int32_t *__restrict__ vin,
                                                         K *__restrict__ kout, int32_t *__restrict__ vout, int64_t n, int shift,
                                                         const uint32_t *__restrict__ offs, unsigned nt)
{
    __shared__ uint32_t base[DD_RADIX];
    __shared__ uint32_t wcnt[DD_BLOCK / 64][DD_RADIX];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
    base[threadIdx.x] = offs[(size_t)threadIdx.x * nt + blockIdx.x];
    const int64_t tile = (int64_t)blockIdx.x * DD_TILE;
    for (int r = 0; r < DD_ITEMS; ++r) {
        for (int q = 0; q < DD_BLOCK / 64; ++q) wcnt[q][threadIdx.x] = 0;
        __syncthreads();
        const int64_t k = tile + r * DD_BLOCK + threadIdx.x;
        const bool valid = k < n;
        const K key = valid ? kin[k] : (K)0;
        const uint32_t d = (uint32_t)(key >> shift) & (DD_RADIX - 1);
        uint64_t same = __ballot(valid);
        for (int b = 0; b < 8; ++b) {
            const uint64_t m = __ballot((d >> b) & 1);
            same &= ((d >> b) & 1) ? m : ~m;
        }
        const uint32_t rank = __popcll(same & below);
        if (valid && rank == 0) wcnt[w][d] = __popcll(same);
        __syncthreads();
        if (valid) {
            uint32_t pos = base[d] + rank;
            for (int q = 0; q < w; ++q) pos += wcnt[q][d];
            kout[pos] = key;
            vout[pos] = vin ? vin[k] : (int32_t)k;
        }
        __syncthreads();
        uint32_t add = 0;
        for (int q = 0; q < DD_BLOCK / 64; ++q) add += wcnt[q][threadIdx.x];
        base[threadIdx.x] += add;             // (read by other threads only after the next barrier)
    }
}

static __global__ void k_dd_iota(int32_t *__restrict__ v, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * DD_BLOCK + threadIdx.x;
    if (i < n) v[i] = (int32_t)i;
}

// scratch of the radix sort for n elements
template <typename K>
struct dd_sort_buf {
    K *k2 = nullptr;
    int32_t *v1 = nullptr, *v2 = nullptr;
    uint32_t *hist = nullptr, *offs = nullptr, *tmp = nullptr;
};

// Stable sort of keys[0..n) on their low `bits` bits; returns the sorted keys and the original index of each (in
// *k_out / *v_out, which point into {keys, b.k2} and {b.v1, b.v2}).  keys are overwritten.
template <typename K>
static void dd_sort(hipStream_t st, K *keys, int64_t n, int bits, const dd_sort_buf<K> &b, K **k_out, int32_t **v_out)
{
    K *ka = keys, *kb = b.k2;
    int32_t *va = nullptr, *vb = b.v1;
    const unsigned nt = dd_grid(n, DD_TILE);
    if (n == 0 || bits == 0) {
        if (n) k_dd_iota<<<dd_grid(n, DD_BLOCK), DD_BLOCK, 0, st>>>(b.v1, n);
        *k_out = keys; *v_out = b.v1;
        return;
    }
    for (int shift = 0; shift < bits; shift += 8) {
        k_dd_hist<K><<<nt, DD_BLOCK, 0, st>>>(ka, n, shift, b.hist, nt);
        dd_scan<uint32_t>(st, b.hist, b.offs, (int64_t)DD_RADIX * nt, b.tmp);
        k_dd_scatter<K><<<nt, DD_BLOCK, 0, st>>>(ka, va, kb, vb, n, shift, b.offs, nt);
        std::swap(ka, kb);
        va = vb;
        vb = vb == b.v1 ? b.v2 : b.v1;
    }
    *k_out = ka; *v_out = va;
}

// one device allocation carved into the scratch arrays of a phase; freed behind the stream
struct dd_arena {
    hipStream_t st = nullptr;
    char *base = nullptr;
    std::vector<std::pair<void **, size_t>> want;
    template <typename T>
    void ask(T **p, int64_t n) { want.push_back({(void **)p, (sizeof(T) * (size_t)std::max<int64_t>(n, 1) + 255) & ~(size_t)255}); }
    hipError_t alloc()
    {
        size_t tot = 0;
        for (auto &w : want) tot += w.second;
        hipError_t e = hipMalloc((void **)&base, tot ? tot : 256);
        if (e != hipSuccess) { base = nullptr; return e; }
        size_t off = 0;
        for (auto &w : want) { *w.first = base + off; off += w.second; }
        return hipSuccess;
    }
    ~dd_arena()
    {
        if (!base) return;
        (void)hipStreamSynchronize(st);
        (void)hipFree(base);
    }
};
