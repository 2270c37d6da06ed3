// Windowed exponential log-likelihood over CHILD SLICES: one lane per child event.
//   λ_c(t_i) = λ0_c(t_i) + Σ_{j<i, t_j > t_i-Δtmax} A[n_j,c] W[n_j,c] θ[n_j,c] exp(-θ[n_j,c] (t_i - t_j))
// (reference: loglikelihood src/continuous.jl:210-239,360-389; total_intensity :286-300 -- the backwards walk from event
//  i-1 that adds one impulse per parent is exactly what a lane does here, most recent parent first).
//
// Mapping to CDNA4
//  * A workgroup owns an item (a run of children of ONE node c): column c of the tables is staged once in LDS as
//    {-θ·unit·64/ln2, a·w·θ} per parent node, entry N = {0, 0} for the padding records.
//  * A wavefront owns a slice = 64 consecutive children of the item (children are sorted by window length, so the 64
//    windows are nearly equal).  Which (parent, child) pairs exist and their delays are data, not parameters; the dataset
//    keeps them slice by slice, ROW r = the r-th most recent parent of each of the 64 children: one wave-wide load fetches a
//    row (256 + 128 contiguous bytes in the two planes of the 6-byte records), every lane keeps its own running sum, and
//    there is no cross-lane reduction, no per-pair predicate and no per-child offset arithmetic at all.
//  * Per evaluation the kernel streams 6 bytes per (padded) pair + 16 bytes per parameter pair: 67 MB at N = 1024, M = 1e6,
//    mean window 8 (the 8-byte list of k_windowed_pairs: 85 MB), and issues ~25 VALU instructions per pair instead of ~44.
//  * Σ log λ from a running mantissa product and exponent sum per lane: multiplied and added across the wave, one logarithm
//    per wave (the shared exit, sl_exit_sums); the fused last-workgroup reduction as in k_windowed.
#include <algorithm>
#include <type_traits>
#include <vector>

#include "nhp_internal.h"
#include "nhp_math.h"
#include "nhp_rng.h"

struct nhp_slices {               // kernel-side view of nhp_cont_dataset::d_sl_*
    const uint32_t *row;          // [n_slices + 1]
    const int32_t *item0;         // [n_items + 1]
    const uint32_t *lo;           // [(rows + 16) * 64]
    const uint16_t *hi;
    int32_t nsh;                  // 16 - node bits: hi = node << nsh | delay >> 32
    uint32_t dmask;               // (1 << nsh) - 1
    int32_t dbits;                // bits of the delay: 32 + nsh
};

#define NHP_SL_SHARDS 64

// C rows of records in registers, and how they are requested ("The row diet").  The rows' base is wave-uniform and
// is formed on the scalar unit; a lane adds its own byte offset (lane·4 in the lo plane, lane·2 in the hi plane) and the C rows
// are immediates: global_load_* v, v_laneoff, s[base:base+1] offset:u·256 -- no 64-bit vector address arithmetic.  The lane
// offsets pass through an empty asm at every request, so that the compiler does not hoist their zero-extended 64-bit copies
// out of the loops and fall back to vector addresses.  The hi plane's 16 bits are zero-extended by the load itself; the
// annotation keeps the extension beside the load (moved behind the loops' phis it becomes a v_and_b32 0xffff at every use).
// Both are ways round what the compiler does today and nothing in the suite sees them fail (the results are the same, the
// instructions come back).  After a compiler update, from csrc/:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -munsafe-fp-atomics --cuda-device-only -S cont_slices.hip -o cont_slices.s
// and in k_slices_batch<512,2,2,true> (_Z14k_slices_batchILi512ELi2ELi2ELb1E...) between the two "Inner Loop Header: Depth=2"
// labels and their back edges there must be no v_lshl_add_u64 and no `v_and_b32 ..., 0xffff`, the record loads must read
// `global_load_dword v, v, s[..:..] offset:256`, and no `s_waitcnt vmcnt(0)` may stand between a "Loop Header: Depth=1" label
// and the inner loop ("The row diet", has the counts to compare with).
typedef const __attribute__((address_space(1))) unsigned char *sl_gbytes;
typedef const __attribute__((address_space(4))) uint32_t *sl_ctab;   // the slice table through the scalar cache: written once, by the dataset builders
template <int C>
struct sl_chunk { uint32_t lo[C], hi[C]; };
template <int C>
__device__ __forceinline__ void sl_request(sl_chunk<C> &q, const uint32_t *plo, const uint16_t *phi, const uint32_t row0, const int r,
                                           uint32_t &lane4, uint32_t &lane2)
{
    const uint64_t o = (uint64_t)row0 + (uint64_t)(uint32_t)r;
    sl_gbytes pl = (sl_gbytes)plo + o * 256, ph = (sl_gbytes)phi + o * 128;
    asm("" : "+s"(pl), "+s"(ph));
    asm volatile("" : "+v"(lane4), "+v"(lane2));
#pragma unroll
    for (int u = 0; u < C; ++u) {
        q.lo[u] = *(const __attribute__((address_space(1))) uint32_t *)(pl + lane4 + u * 256);
        q.hi[u] = __builtin_annotation((uint32_t)*(const __attribute__((address_space(1))) uint16_t *)(ph + lane2 + u * 128), "zext");
    }
}

#ifdef NHP_STAMP      // diagnostic build only (tools/dbg/slstamps.py): s_memrealtime (100 MHz, one clock for all XCDs) at the phase boundaries of wave 0 of every workgroup
__device__ unsigned long long g_sl_stamps[8 * 4096];
__device__ unsigned long long g_sl_wave_end[16 * 4096];      // and of EVERY wave at the end of its slices (0: the workgroup has no such wave)
#define NHP_SL_STAMP(i) do { if (threadIdx.x == 0 && blockIdx.x < 4096) g_sl_stamps[8 * blockIdx.x + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define NHP_SL_STAMP_WAVE() do { if ((threadIdx.x & 63) == 0 && blockIdx.x < 4096) g_sl_wave_end[16 * blockIdx.x + (threadIdx.x >> 6)] = __builtin_amdgcn_s_memrealtime(); } while (0)
extern "C" int nhp_debug_stamps_slices(unsigned long long *out, int n)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sl_stamps), sizeof(unsigned long long) * (size_t)n);
}
extern "C" int nhp_debug_stamps_slices_waves(unsigned long long *out, int n)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sl_wave_end), sizeof(unsigned long long) * (size_t)n);
}
#else
#define NHP_SL_STAMP(i) do { } while (0)
#define NHP_SL_STAMP_WAVE() do { } while (0)
#endif

// the dealing of slices to waves as the kernels below compute it, for a host test
extern "C" int32_t nhp_debug_slice_of(int32_t round, int32_t wave, int32_t nw) { return nhp_slice_of(round, wave, nw); }

__device__ __forceinline__ double sl_baseline(const nhp_cont_args &a, int c, double t)
{
#pragma clang fp contract(off)
    if (a.baseline_kind == NHP_BASELINE_HOMOGENEOUS) return a.lambda0[c];
    const double *x = a.grid;
    const double *y = a.lambda0 + (size_t)c * a.grid_n;
    int lo = 0, hi = a.grid_n - 1;
    if (!(t < x[hi])) return y[hi];
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t >= x[mid]) lo = mid; else hi = mid;
    }
    return (y[lo + 1] * (t - x[lo]) + y[lo] * (x[lo + 1] - t)) / (x[lo + 1] - x[lo]);
}

// -∫λ0_c: λ·duration (src/baselines.jl:98-102) or the trapezoid rule over the grid, which ignores `duration`
// (src/baselines.jl:336); spread over the threads of the workgroup (their block sum adds it up)
__device__ __forceinline__ double sl_baseline_integral_col(const nhp_cont_args &a, int c)
{
    if (a.baseline_kind == NHP_BASELINE_HOMOGENEOUS) return threadIdx.x == 0 ? a.lambda0[c] * a.duration : 0.0;
    const double *y = a.lambda0 + (size_t)c * a.grid_n;
    double I = 0.0;
    for (int i = threadIdx.x; i + 1 < a.grid_n; i += blockDim.x) I += 0.5 * (y[i] + y[i + 1]) * (a.grid[i + 1] - a.grid[i]);
    return I;
}

// ∂ log λ_i / ∂(grid intensities of node c) for an event at time t: g = 1/λ_i spread over the two grid neighbours with the
// interpolation weights (src/utils/interpolation.jl:26-35); as grad_lgcp_scatter of cont_grad.hip
__device__ __forceinline__ void sl_lgcp_scatter(const nhp_cont_args &a, int c, double t, double g, double *grad)
{
    const double *x = a.grid;
    const int G = a.grid_n;
    double *gc = grad + (size_t)c * G;
    int lo = 0, hi = G - 1;
    if (!(t < x[hi])) { atomicAdd(&gc[hi], g); return; }
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t >= x[mid]) lo = mid; else hi = mid;
    }
    const double w = x[lo + 1] - x[lo];
    atomicAdd(&gc[lo], g * (x[lo + 1] - t) / w);
    atomicAdd(&gc[lo + 1], g * (t - x[lo]) / w);
}

// Fills the planes: wave = slice, lane = child, row r = the child's r-th most recent parent (src/continuous.jl:290-298 walks
// the window in this order).  Delays are rounded to 2^-dbits of Δtmax and kept inside [1, 2^dbits - 1] (a tie Δt = 0 becomes
// one unit: 7e-12·Δtmax at N = 1024); rows past a child's window hold {node N, delay 0}.
__global__ __launch_bounds__(256) void k_slices_build(nhp_cont_args a, nhp_slices sl, uint32_t *__restrict__ lo, uint16_t *__restrict__ hi)
{
    const nhp_item it = a.items[blockIdx.x];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nchild = it.kend - it.kbeg;
    const int s0 = sl.item0[blockIdx.x], ns = sl.item0[blockIdx.x + 1] - s0;
    const double two_d = __builtin_ldexp(1.0, sl.dbits);
    const double scale = a.inv_dtmax * two_d, qmax = two_d - 1.0;
    for (int j = w; j < ns; j += 4) {
        const uint32_t row0 = sl.row[s0 + j];
        const int K = (int)(sl.row[s0 + j + 1] - row0);
        const int kk = 64 * j + lane;
        nhp_child ch;
        ch.t = 0.0; ch.first = 0; ch.idx = 0;
        if (kk < nchild) ch = a.child_w[it.kbeg + kk];
        const int len = ch.idx - ch.first;
        for (int r = 0; r < K; ++r) {
            uint32_t l = 0, h = (uint32_t)a.N << sl.nsh;
            if (r < len) {
                const nhp_event e = a.ev[ch.idx - 1 - r];
                double q = __builtin_rint((ch.t - e.t) * scale);
                q = q < 1.0 ? 1.0 : (q > qmax ? qmax : q);
                const uint64_t qi = (uint64_t)q;
                l = (uint32_t)qi;
                h = ((uint32_t)e.node << sl.nsh) | (uint32_t)(qi >> 32);
            }
            const size_t o = ((size_t)row0 + (size_t)r) * 64 + (size_t)lane;
            lo[o] = l;
            hi[o] = (uint16_t)h;
        }
    }
}

struct nhp_pslices {              // kernel-side view of the parent slices (nhp_cont_dataset::d_ps_*) + where the gradient goes
    const uint32_t *row;          // [n_items * spi + 1]
    const uint16_t *perm;         // [n_items * spi * 64]
    const uint32_t *lo;
    const uint16_t *hi;
    int32_t spi;                  // parent slices per item
    int32_t psh;                  // 16 - slot bits: hi = slot << psh | delay >> 32
    uint32_t dmask;
    int32_t dbits;
    int32_t max_item;             // the padding records' slot (its 1/λ is 0)
    int32_t direct;               // every item is its node's only one, whole dataset, flat baseline: the gradient is stored, not added
    double *grad;                 // [P] params! order
};

// pairs of every item by parent node: cnt[item * N + p]
__global__ __launch_bounds__(256) void k_ps_count(nhp_cont_args a, uint32_t *__restrict__ cnt)
{
    extern __shared__ __align__(16) unsigned char smem[];
    uint32_t *hist = reinterpret_cast<uint32_t *>(smem);
    const nhp_item it = a.items[blockIdx.x];
    for (int p = threadIdx.x; p < a.N; p += 256) hist[p] = 0;
    __syncthreads();
    for (int k = it.kbeg + threadIdx.x; k < it.kend; k += 256) {
        const nhp_child ch = a.child_w[k];
        for (int j = ch.idx - 1; j >= ch.first; --j) atomicAdd(&hist[a.ev[j].node], 1u);
    }
    __syncthreads();
    for (int p = threadIdx.x; p < a.N; p += 256) cnt[(size_t)blockIdx.x * a.N + p] = hist[p];
}

// the item's parent nodes by pair count (most first, ties by node): lane order of the parent slices, rows of every slice
__global__ __launch_bounds__(256) void k_ps_rank(int N, int spi, const uint32_t *__restrict__ cnt, uint16_t *__restrict__ perm,
                                                 uint16_t *__restrict__ rankof, uint32_t *__restrict__ rows)
{
    extern __shared__ __align__(16) unsigned char smem[];
    uint32_t *c = reinterpret_cast<uint32_t *>(smem);
    for (int p = threadIdx.x; p < N; p += 256) c[p] = cnt[(size_t)blockIdx.x * N + p];
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * spi * 64;
    for (int p = threadIdx.x; p < N; p += 256) {
        const uint32_t mine = c[p];
        int rank = 0;
        for (int q = 0; q < N; ++q) rank += (c[q] > mine || (c[q] == mine && q < p)) ? 1 : 0;
        perm[base + rank] = (uint16_t)p;
        rankof[(size_t)blockIdx.x * N + p] = (uint16_t)rank;
        if ((rank & 63) == 0) rows[(size_t)blockIdx.x * spi + (rank >> 6)] = mine;
    }
    for (int q = N + threadIdx.x; q < spi * 64; q += 256) perm[base + q] = 0xFFFFu;
}

// every pair into its parent's lane (position by an LDS ticket: any order), then the rest of the lane padded
__global__ __launch_bounds__(256) void k_ps_fill(nhp_cont_args a, nhp_pslices ps, const uint32_t *__restrict__ cnt, const uint16_t *__restrict__ rankof,
                                                 uint32_t *__restrict__ lo, uint16_t *__restrict__ hi)
{
    extern __shared__ __align__(16) unsigned char smem[];
    uint32_t *cursor = reinterpret_cast<uint32_t *>(smem);
    const nhp_item it = a.items[blockIdx.x];
    const int N = a.N;
    for (int p = threadIdx.x; p < N; p += 256) cursor[p] = 0;
    __syncthreads();
    const double two_d = __builtin_ldexp(1.0, ps.dbits);
    const double scale = a.inv_dtmax * two_d, qmax = two_d - 1.0;
    const uint32_t *row = ps.row + (size_t)blockIdx.x * ps.spi;
    for (int k = it.kbeg + threadIdx.x; k < it.kend; k += 256) {
        const nhp_child ch = a.child_w[k];
        const uint32_t slot = (uint32_t)(k - it.kbeg);
        for (int j = ch.idx - 1; j >= ch.first; --j) {
            const nhp_event e = a.ev[j];
            const uint32_t pos = atomicAdd(&cursor[e.node], 1u);
            const int rk = rankof[(size_t)blockIdx.x * N + e.node];
            double q = __builtin_rint((ch.t - e.t) * scale);
            q = q < 1.0 ? 1.0 : (q > qmax ? qmax : q);
            const uint64_t qi = (uint64_t)q;
            const size_t o = ((size_t)row[rk >> 6] + pos) * 64 + (size_t)(rk & 63);
            lo[o] = (uint32_t)qi;
            hi[o] = (uint16_t)((slot << ps.psh) | (uint32_t)(qi >> 32));
        }
    }
    // lanes shorter than their slice, and the lanes behind the last node
    for (int rk = threadIdx.x; rk < ps.spi * 64; rk += 256) {
        const int p = ps.perm[(size_t)blockIdx.x * ps.spi * 64 + rk];
        const uint32_t n = p == 0xFFFF ? 0u : cnt[(size_t)blockIdx.x * N + p];
        const uint32_t r0 = row[rk >> 6], R = row[(rk >> 6) + 1] - r0;
        for (uint32_t i = n; i < R; ++i) {
            const size_t o = ((size_t)r0 + i) * 64 + (size_t)(rk & 63);
            lo[o] = 0;
            hi[o] = (uint16_t)((uint32_t)ps.max_item << ps.psh);
        }
    }
}

// every lane's records sorted by (slot, delay): the list is the same whatever order the tickets were drawn in
__global__ __launch_bounds__(256) void k_ps_sort(int N, nhp_pslices ps, const uint32_t *__restrict__ cnt, uint32_t *__restrict__ lo,
                                                 uint16_t *__restrict__ hi)
{
    const uint32_t *row = ps.row + (size_t)blockIdx.x * ps.spi;
    for (int rk = threadIdx.x; rk < ps.spi * 64; rk += 256) {
        const int p = ps.perm[(size_t)blockIdx.x * ps.spi * 64 + rk];
        if (p == 0xFFFF) continue;
        const int n = (int)cnt[(size_t)blockIdx.x * N + p];
        const size_t o0 = (size_t)row[rk >> 6] * 64 + (size_t)(rk & 63);
        for (int i = 1; i < n; ++i) {
            const uint32_t l = lo[o0 + (size_t)i * 64], h = hi[o0 + (size_t)i * 64];
            const uint64_t key = ((uint64_t)h << 32) | l;
            int j = i - 1;
            while (j >= 0) {
                const uint32_t lj = lo[o0 + (size_t)j * 64], hj = hi[o0 + (size_t)j * 64];
                if ((((uint64_t)hj << 32) | lj) <= key) break;
                lo[o0 + (size_t)(j + 1) * 64] = lj;
                hi[o0 + (size_t)(j + 1) * 64] = (uint16_t)hj;
                --j;
            }
            lo[o0 + (size_t)(j + 1) * 64] = l;
            hi[o0 + (size_t)(j + 1) * 64] = (uint16_t)h;
        }
    }
}

// ---- the exit every exponential log-likelihood kernel of this file shares ------------------------------------------
// A workgroup leaves two numbers per model: Σ log λ over its children and its share of the integral.  Both are formed HERE for
// k_windowed_slices (fused and deferred exit) and k_slices_batch (every S, DEFER or not), so the routes the tests hold to each
// other with `==` agree by construction.  Q = S·NW (model, wave) pairs, q = m·NW + w; behind the 2^(j/64) table the kernels keep
//   park [Q][17]  the integral's partial sums, one per quad of lanes (16 a wave; the 17th pads the banks for the read below)
//   qman [Q][17]  the wave's mantissa products, one per quad of lanes, each in [2^-4, 1)
//   qexp [Q][17]  the quads' exponent sums (int32)
// Σ log λ: a lane carries a mantissa product and an exponent sum over its children.  A wave multiplies the mantissas of every
// quad of lanes (two DPP steps: lanes i and i^1, then the pairs) and adds the quad's exponents as integers, and the lanes with
// (lane & 3) == 0 park the 16 products and 16 sums of (model, wave).  After the barrier lane q of the first wave multiplies the 16
// of (model, wave) q in lane order (16 factors >= 2^-4 stay >= 2^-64: no underflow), adds the 16 exponents, renormalises once
// with frexp and takes ONE logarithm; thread 0 adds the logarithms wave by wave.
// A lane without a child holds {1.0, 0} and changes nothing; a wave without a slice leaves {0.5, 1}: log 0.5 + ln 2 is exactly 0
// (nhp_log's ln2_hi + ln2_lo rounds to the constant below).  A child with λ = 0 makes the product 0 and the sum -inf, one
// with λ < 0 made its mantissa NaN in the row loop.
// The integral: a wave stops its sum after the two quad steps, in the head, and parks 16 partial sums; lane q of the first wave
// adds the 16 of (model, wave) q in lane order at the exit, where it is alone anyway, and thread 0 adds the waves' sums in wave
// order.  Nothing of the integral is live in the row loop.
__host__ __device__ constexpr size_t sl_exit_bytes(const int S, const int NW) { return ((size_t)S * NW * (17 * 8 + 17 * 8 + 17 * 4) + 15) / 16 * 16; }

// What a workgroup of `block` threads with the columns of S models takes: the block sums' words, the columns, the 2^(j/64)
// table, the shared exit's area for the waves actually launched.  Every launcher and the pairing rule take this one line.
static inline size_t sl_lds_bytes(const int N, const int S, const int block)
{
    return 320 + 16 * ((size_t)N + 1) * (size_t)S + 512 + sl_exit_bytes(S, block / 64);
}

// The pair term of k_slices_batch and k_windowed_slices<., ., ., GRAD = false> is nhp_exp_term_fast / _slow (nhp_math.h) on the
// table's BIASED entries; the gradient build, the logit-normal and sampler kernels keep nhp_exp_neg_tab_scaled and the plain ones.
// Which path the item's terms take (nhp_math.h: the limit).  Every thread compares the column entries IT forms with
// sl_term_limit -- `bad` is true for |cx| above it, NaN and +-inf -- a wave leaves the OR of its lanes in flg[wave] before the
// head's barrier, and behind it every wave reads all NW words: one wave-uniform answer per workgroup, for every model of the pass.
// flg = the block sums' words, which nothing touches before the exit's barrier.
__device__ __forceinline__ double sl_term_limit(const int dbits) { return __builtin_ldexp(NHP_EXP_TERM_LIMIT, -dbits); }
__device__ __forceinline__ bool sl_term_outside(const double cx, const double lim) { return !(__builtin_fabs(cx) <= lim); }
__device__ __forceinline__ void sl_limit_post(const bool bad, int *__restrict__ flg, const int w, const int lane)
{
    const bool any = __builtin_amdgcn_ballot_w64(bad) != 0;
    if (lane == 0) flg[w] = any ? 1 : 0;
}
template <int NW>
__device__ __forceinline__ bool sl_limit_all_inside(const int *__restrict__ flg, const int lane)
{
    return __builtin_amdgcn_ballot_w64(flg[lane & (NW - 1)] != 0) == 0;
}

__device__ __forceinline__ double sl_dpp_mul(const double v, const int sel)
{
#pragma clang fp contract(off)
    const int lo = __double2loint(v), hi = __double2hiint(v);
    int plo, phi;
    if (sel == 0) { plo = __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xF, 0xF, true); phi = __builtin_amdgcn_mov_dpp(hi, 0xB1, 0xF, 0xF, true); }   // quad_perm [1,0,3,2]
    else { plo = __builtin_amdgcn_mov_dpp(lo, 0x4E, 0xF, 0xF, true); phi = __builtin_amdgcn_mov_dpp(hi, 0x4E, 0xF, 0xF, true); }          // quad_perm [2,3,0,1]
    return v * __hiloint2double(phi, plo);
}

// the head's half of the integral: v = this thread's terms of model m
template <int NW>
__device__ __forceinline__ void sl_exit_park(double v, double *__restrict__ park, const int m, const int w, const int lane)
{
#pragma clang fp contract(off)
    v = nhp_dpp_add(v, 0);
    v = nhp_dpp_add(v, 1);
    if ((lane & 3) == 0) park[(m * NW + w) * 17 + (lane >> 2)] = v;
}

// Every thread calls it once, after its last slice; the integral's partial sums were parked before an earlier barrier.  Thread 0
// returns with sx[m] = Σ log λ and sy[m] = the integral's share of the workgroup; the other threads' values mean nothing.
template <int NW, int S>
__device__ __forceinline__ void sl_exit_sums(const double (&prod)[S], const int (&pexp)[S], double *__restrict__ park, double (&sx)[S], double (&sy)[S])
{
#pragma clang fp contract(off)
    constexpr int Q = S * NW;
    static_assert(Q <= 64, "one lane of the first wave per (model, wave)");
    double *qman = park + Q * 17;
    int *qexp = reinterpret_cast<int *>(qman + Q * 17);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    double p[S];
    int e[S];
#pragma unroll
    for (int m = 0; m < S; ++m) {
        p[m] = sl_dpp_mul(sl_dpp_mul(prod[m], 0), 1);
        e[m] = pexp[m];
        e[m] += __builtin_amdgcn_mov_dpp(e[m], 0xB1, 0xF, 0xF, true);
        e[m] += __builtin_amdgcn_mov_dpp(e[m], 0x4E, 0xF, 0xF, true);
    }
    int ql = lane;                                                  // (formed here: taken from the head's parking address it would
    asm volatile("" : "+v"(ql));                                    //  stay in two registers through the row loop)
    if ((ql & 3) == 0) {
        const int o = w * 17 + (ql >> 2);
#pragma unroll
        for (int m = 0; m < S; ++m) {
            qman[m * NW * 17 + o] = p[m];
            qexp[m * NW * 17 + o] = e[m];
        }
    }
    __syncthreads();
    if (w != 0) return;                                             // (the helper's end: the callers' exits go on)
    if (lane < Q) {
        double *pm = qman + lane * 17;
        const int *pe = qexp + lane * 17;
        double *pk = park + lane * 17;
        // (three groups of 16 loads, each used up before the next is requested: all 48 in flight under the logarithm would set
        //  the kernel's register count)
        double r = pm[0], si = 0.0;
        int es = pe[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) r *= pm[i];
        asm volatile("" : "+v"(r) : : "memory");
#pragma unroll
        for (int i = 1; i < 16; ++i) es += pe[i];
        asm volatile("" : "+v"(es) : : "memory");
#pragma unroll
        for (int i = 0; i < 16; ++i) si += pk[i];
        asm volatile("" : "+v"(si) : : "memory");
        es += __builtin_amdgcn_frexp_exp(r);
        const double lg = nhp_log(__builtin_amdgcn_frexp_mant(r)) + (double)es * 6.93147180559945286e-01;
        pm[0] = lg;                                                 // (each lane its own entries, read above by itself only)
        pk[0] = si;
    }
    // the first wave alone: its LDS operations complete in order, the fences keep the compiler from moving them
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (tid == 0) {
#pragma unroll
        for (int m = 0; m < S; ++m) {
            double x = 0.0, y = 0.0;
            for (int q = 0; q < NW; ++q) { x += qman[(m * NW + q) * 17]; y += park[(m * NW + q) * 17]; }
            sx[m] = x; sy[m] = y;
        }
    }
}

// C rows of a slice are requested at a time into one of two register sets: the next set is in flight while this one is
// summed, across slice boundaries too (the first rows of a wave's next slice are requested under the last rows of this one,
// and the very first set before the column is staged: its addresses need the slice table only).
// GRAD: the analytic gradient in the same launch (the objective of mle!, src/continuous.jl:144-198, differentiated by hand;
// formulas at the top of cont_grad.hip).  `out` null: the block sums only, without the baseline's integral (the caller adds it up
// and owns that term).  `defer` (with `out` given, the enqueue route): the whole evaluation's block sums, baseline integral
// included, into `partials` -- here a result slot's own buffer -- and no second stage: k_finalize_slots adds them at the join.  Phase A is the log-likelihood itself and leaves g_k = 1/λ_k of the item's children
// in LDS; phase B walks the item's PARENT slices -- lane = parent node p, its θ[p,c], W[p,c] in registers, row r = the node's
// r-th pair as {child slot, delay} -- and every lane sums Σ g·e^{-θΔ} and Σ g·(1-θΔ)·e^{-θΔ} over its own pairs: no atomics,
// no cross-lane step, the list streamed once.  An item that is its node's only one stores the column's gradient (the
// parameter-independent terms included), others add to what k_grad_init left.
template <int BLOCK, int C, bool FLAT, bool GRAD>
__global__ __launch_bounds__(BLOCK) void k_windowed_slices(nhp_cont_args a, nhp_slices sl, nhp_pslices ps, int mask_integral,
                                                            double *__restrict__ partials, unsigned int *__restrict__ counter,
                                                            double *__restrict__ out, int defer)
{
    constexpr int NW = BLOCK / 64;
    extern __shared__ __align__(16) unsigned char smem[];
    double *red = reinterpret_cast<double *>(smem);                 // [2 * NW <= 32] + flag at [32]
    double2 *col = reinterpret_cast<double2 *>(smem + 320);         // [N + 1] {-θ·unit·64/ln2, a·w·θ}; [N] = {0, 0}
    double *etab = reinterpret_cast<double *>(col + a.N + 1);       // [64] 2^(j/64); !GRAD: biased (nhp_exp_tab_biased)
    double *ginv = etab + 64;                                       // GRAD: [max_item + 1] 1/λ of the item's children; [max_item] = 0
    double *park = etab + 64;                                       // !GRAD: the shared exit's sums (sl_exit_bytes(1, NW))
    const int tid = threadIdx.x, lane = tid & 63;
    const double tab_v = nhp_exp2_64[lane];                         // requested first, parked in LDS with the column (one wait)

    const nhp_item it = a.items[blockIdx.x];
    const int c = it.node, N = a.N;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nchild = it.kend - it.kbeg;
    const int s0 = sl.item0[blockIdx.x], ns = sl.item0[blockIdx.x + 1] - s0;
    NHP_SL_STAMP(0);

    // Rows r .. r+C-1 of the slice that starts at row `row0`: a wave-uniform base and compile-time row offsets.  Rows past the
    // slice's last are simply the next slice's (or the 16 rows of padding behind the list): loaded, never summed.
    typedef sl_chunk<C> chunk;
    uint32_t lane4 = (uint32_t)lane * 4u, lane2 = (uint32_t)lane * 2u;
    // (the gradient build keeps vector addresses and vector loads of the slice table: its phase B holds the scalar registers)
    auto request = [&](chunk &q, const uint32_t *plo, const uint16_t *phi, const uint32_t row0, const int r) {
        if constexpr (GRAD) {
            const size_t o = ((size_t)row0 + (size_t)r) * 64;
            const uint32_t *pl = plo + o;
            const uint16_t *ph = phi + o;
#pragma unroll
            for (int u = 0; u < C; ++u) {
                q.lo[u] = pl[u * 64 + lane];
                q.hi[u] = ph[u * 64 + lane];
            }
        } else sl_request<C>(q, plo, phi, row0, r, lane4, lane2);
    };
    auto rowc = [&](const int i) {
        if constexpr (GRAD) return sl.row[i];
        else return ((sl_ctab)sl.row)[i];
    };
    // Column c of the tables: every load of (up to) UN passes over the parent nodes is requested before any is used -- one
    // round trip instead of one per pass -- and the first rows of the wave's first slice are requested right behind them
    // (their addresses need the slice table only), so they arrive while the column is being written to LDS.
    constexpr int UN = BLOCK >= 512 ? 2 : 4;
    const double unit = __builtin_ldexp(a.dt_max, -sl.dbits);      // Δtmax · 2^-dbits
    const double tlim = GRAD ? 0.0 : sl_term_limit(sl.dbits);
    bool outside = false;
    int j = w;
    uint32_t row0 = 0;
    int K = 0;
    chunk qa, qb;
    double integ = 0.0;
    for (int p0 = 0; p0 < N; p0 += UN * BLOCK) {
        double w_[UN], th_[UN], a_[UN], cnt_[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int p = p0 + u * BLOCK + tid;
            const size_t k = (size_t)(p < N ? p : 0) + (size_t)c * N;
            w_[u] = a.W[k];
            th_[u] = a.p1[k];
            a_[u] = a.A ? a.A[k] : 1.0;
            cnt_[u] = it.first ? a.cnt[p < N ? p : 0] : 0.0;
        }
        if (p0 == 0) {
            if (j < ns) { row0 = rowc(s0 + j); K = (int)(rowc(s0 + j + 1) - row0); }
            asm volatile("" ::: "memory");
            request(qa, sl.lo, sl.hi, row0, 0);
            asm volatile("" ::: "memory");
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int p = p0 + u * BLOCK + tid;
            if (p < N) {
                double wv = w_[u], wint = wv;
                if (a.A) {
                    wv = a_[u] * wv;
                    if (mask_integral) wint = wv;
                }
                col[p] = make_double2(-((th_[u] * unit) * 92.33248261689366), wv * th_[u]);   // term = (a·w·θ)·exp(-(θ·unit)·q), the rate times 64/ln 2
                if constexpr (!GRAD) outside |= sl_term_outside(-((th_[u] * unit) * 92.33248261689366), tlim);
                integ += cnt_[u] * wint;
            }
        }
    }
    if (tid < 64) etab[tid] = GRAD ? tab_v : nhp_exp_tab_biased(tab_v, tid);
    if (tid == 0) col[N] = make_double2(0.0, 0.0);
    if (GRAD && tid == 0) ginv[ps.max_item] = 0.0;
    if (out && it.first) integ += sl_baseline_integral_col(a, c);
    if constexpr (!GRAD) {
        sl_exit_park<NW>(integ, park, 0, w, lane);                  // (the gradient build keeps its own exit: DESIGN 3.1d)
        sl_limit_post(outside, reinterpret_cast<int *>(red), w, lane);
    }
    __syncthreads();
    NHP_SL_STAMP(1);
    const bool fast = GRAD ? false : sl_limit_all_inside<NW>(reinterpret_cast<const int *>(red), lane);

    const double lam0 = FLAT ? a.lambda0[c] : 0.0;
    const uint32_t dmask = sl.dmask;
    const int nsh = sl.nsh;
    const nhp_exp_term_consts ekc = nhp_exp_term_setup();
    // the high delay bits under the exponent of 2^52 (one v_bfi_b32): the double 2^52 + delay, minus 2^52
    auto delay = [&](const uint32_t lo, const uint32_t h, const uint32_t mask) {
        uint32_t hw;
        asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(hw) : "s"(mask), "v"(h), "v"(0x43300000u));
        return __hiloint2double((int)hw, (int)lo) - 4503599627370496.0;
    };
    // A term, once per way of forming it: MODE 0 the gradient build's (nhp_exp_neg_tab_scaled: phase B shares its table), 1 and 2
    // the fast and the slow path of nhp_exp_term -- chosen per slice by ONE wave-uniform branch, outside the row loop.
    auto term = [&](auto mode, const uint32_t lo, const uint32_t h) {
        constexpr int MODE = decltype(mode)::value;
        const double v = delay(lo, h, dmask);
        const double2 cw = col[h >> nsh];
        if constexpr (MODE == 0) return cw.y * nhp_exp_neg_tab_scaled(cw.x * v, etab);
        else if constexpr (MODE == 1) return cw.y * nhp_exp_term_fast(cw.x, v, etab, ekc);
        else return cw.y * nhp_exp_term_slow(cw.x, v, etab, ekc);
    };
    // A request that lies wholly inside the slice is summed as C independent straight-line chains (their LDS round trips --
    // column entry, then the table's entry -- overlap); the slice's last request goes row by row behind wave-uniform
    // branches.  The sum itself is sequential in both: most recent parent first, the reference's order.
    // (The slow path goes row by row throughout: summed as chains, its longer terms would set the kernel's register count.)
    auto sum = [&](auto mode, const chunk &q, const int r, const int K, double s) {
        constexpr int MODE = decltype(mode)::value;
        if (MODE != 2 && r + C <= K) {
            double t[C];
#pragma unroll
            for (int u = 0; u < C; ++u) t[u] = term(mode, q.lo[u], q.hi[u]);
#pragma unroll
            for (int u = 0; u < C; ++u) s += t[u];
        } else {
#pragma unroll
            for (int u = 0; u < C; ++u)
                if (r + u < K) s += term(mode, q.lo[u], q.hi[u]);
        }
        return s;
    };
    // the rows of one slice, the next slice's first request under its last rows (a macro, not a lambda: the gradient build's
    // instructions stay what they were before there were three modes)
#define NHP_SL_ROWS(mode)                                                                                             \
    for (int r0 = 0; r0 < K; r0 += 2 * C) {                                                                           \
        request(qb, sl.lo, sl.hi, row0, r0 + C);                                                                      \
        asm volatile("" ::: "memory");                                                                                \
        s = sum(mode, qa, r0, K, s);                                                                                  \
        const bool more = r0 + 2 * C < K;                                                                             \
        request(qa, sl.lo, sl.hi, more ? row0 : row0n, more ? r0 + 2 * C : 0);                                        \
        asm volatile("" ::: "memory");                                                                                \
        s = sum(mode, qb, r0 + C, K, s);                                                                              \
    }
    double prod = 1.0, gsum = 0.0;
    int pexp = 0;
    int rnd = 0;                                                    // the wave's slices in snake order (nhp_slice_of)
    while (j < ns) {
        const int jn = nhp_slice_of(++rnd, w, NW);
        // (a scalar load, waited for where row0n is first used; past the wave's last slice it reads the item's last entry: a
        //  valid row for the request below, which nothing sums, and K is not used again)
        const int jc = s0 + (jn < ns ? jn : ns - 1);
        const uint32_t row0n = rowc(jc), rowen = rowc(jc + 1);
        double s = 0.0;
        if (K <= 0) request(qa, sl.lo, sl.hi, row0n, 0);
        if constexpr (GRAD) { NHP_SL_ROWS((std::integral_constant<int, 0>{})) }
        else if (fast) { NHP_SL_ROWS((std::integral_constant<int, 1>{})) }
        else { NHP_SL_ROWS((std::integral_constant<int, 2>{})) }
#undef NHP_SL_ROWS
        const int kk = 64 * j + lane;
        if (kk < nchild) {
            const double tk = FLAT ? 0.0 : a.child_w[it.kbeg + kk].t;
            const double lam = (FLAT ? lam0 : sl_baseline(a, c, tk)) + s;
            prod *= lam < 0.0 ? __builtin_nan("") : __builtin_amdgcn_frexp_mant(lam);
            pexp += __builtin_amdgcn_frexp_exp(lam);
            if (GRAD) {
                const double g = 1.0 / lam;
                ginv[kk] = g;
                if (FLAT) gsum += g;
                else sl_lgcp_scatter(a, c, tk, g, ps.grad);
            }
        }
        pexp += __builtin_amdgcn_frexp_exp(prod);
        prod = __builtin_amdgcn_frexp_mant(prod);
        j = jn; row0 = row0n; K = (int)(rowen - row0n);
    }
    NHP_SL_STAMP_WAVE();
    NHP_SL_STAMP(2);
    if (GRAD) {
        // ---- phase B: the item's pairs by parent node ----
        const uint32_t *prow = ps.row + (size_t)blockIdx.x * ps.spi;
        const uint16_t *pperm = ps.perm + (size_t)blockIdx.x * ps.spi * 64;
        const double punit = __builtin_ldexp(a.dt_max, -ps.dbits);
        const uint32_t pmask = ps.dmask;
        const int psh = ps.psh;
        const nhp_layout L(a);                                      // (exponential impulses: W follows θ)
        // a lane's node and its parameters, requested a slice ahead
        struct lanep { int p; double th, wv, av, cn; };
        auto lane_params = [&](const int jj) {
            lanep q;
            q.p = jj < ps.spi ? (int)pperm[jj * 64 + lane] : 0xFFFF;
            const size_t k = (size_t)(q.p == 0xFFFF ? 0 : q.p) + (size_t)c * N;
            q.th = a.p1[k];
            q.wv = a.W[k];
            q.av = a.A ? a.A[k] : 1.0;
            q.cn = ps.direct ? a.cnt[q.p == 0xFFFF ? 0 : q.p] : 0.0;
            return q;
        };
        int jp = w;
        uint32_t prow0 = 0;
        int Kp = 0;
        if (jp < ps.spi) { prow0 = prow[jp]; Kp = (int)(prow[jp + 1] - prow0); }
        lanep cur = lane_params(jp);
        request(qa, ps.lo, ps.hi, prow0, 0);
        __syncthreads();                                            // every wave's g_k are in LDS
        auto gterm = [&](const uint32_t lo, const uint32_t h, const double xs, double &accH, double &acc1) {
            const double v = delay(lo, h, pmask);
            const double g = ginv[h >> psh];
            const double t = xs * v;
            const double ge = g * nhp_exp_neg_tab_scaled(t, etab);
            accH += ge;                                             // Σ g·e^{-θΔ}
            acc1 = __builtin_fma(ge, __builtin_fma(t, 1.0830424696249145e-02, 1.0), acc1);   // Σ g·(1 - θΔ)·e^{-θΔ}; θΔ = -t·ln2/64
        };
        auto gsum_chunk = [&](const chunk &q, const int r, const int K, const double xs, double &accH, double &acc1) {
            if (r + C <= K) {
#pragma unroll
                for (int u = 0; u < C; ++u) gterm(q.lo[u], q.hi[u], xs, accH, acc1);
            } else {
#pragma unroll
                for (int u = 0; u < C; ++u)
                    if (r + u < K) gterm(q.lo[u], q.hi[u], xs, accH, acc1);
            }
        };
        while (jp < ps.spi) {
            const int jn = jp + NW;
            uint32_t row0n = 0;
            int Kn = 0;
            if (jn < ps.spi) { row0n = prow[jn]; Kn = (int)(prow[jn + 1] - row0n); }
            const lanep nxt = lane_params(jn);
            const double xs = -((cur.th * punit) * 92.33248261689366);
            double accH = 0.0, acc1 = 0.0;
            if (Kp <= 0) request(qa, ps.lo, ps.hi, row0n, 0);
            for (int r0 = 0; r0 < Kp; r0 += 2 * C) {
                request(qb, ps.lo, ps.hi, prow0, r0 + C);
                asm volatile("" ::: "memory");
                gsum_chunk(qa, r0, Kp, xs, accH, acc1);
                const bool more = r0 + 2 * C < Kp;
                request(qa, ps.lo, ps.hi, more ? prow0 : row0n, more ? r0 + 2 * C : 0);
                asm volatile("" ::: "memory");
                gsum_chunk(qb, r0 + C, Kp, xs, accH, acc1);
            }
            if (cur.p != 0xFFFF) {
                const size_t k = (size_t)cur.p + (size_t)c * N;
                const double gW = cur.av * (cur.th * accH);         // ∂/∂W[p,c]: a Σ g·θ e^{-θΔ}
                const double gT = (cur.av * cur.wv) * acc1;         // ∂/∂θ[p,c]: a·w Σ g·(1 - θΔ) e^{-θΔ}
                if (ps.direct) {
                    const double mk = (a.A && mask_integral) ? cur.av : 1.0;
                    ps.grad[L.W + k] = gW - cur.cn * mk;
                    ps.grad[L.p1 + k] = gT;
                } else {
                    if (gW != 0.0) atomicAdd(&ps.grad[L.W + k], gW);
                    if (gT != 0.0) atomicAdd(&ps.grad[L.p1 + k], gT);
                }
            }
            jp = jn; prow0 = row0n; Kp = Kn; cur = nxt;
        }
    }
    double blk = 0.0, blk_int = 0.0;
    if constexpr (GRAD) {
        double acc = nhp_log(prod) + (double)pexp * 6.93147180559945286e-01;
        if (prod == 0.0) acc = -__builtin_inf();
        blk = acc; blk_int = integ;
        nhp_block_sum2_n<NW>(blk, blk_int, red);
    } else {
        const double p1[1] = {prod};
        const int e1[1] = {pexp};
        double sx[1] = {0.0}, sy[1] = {0.0};
        sl_exit_sums<NW, 1>(p1, e1, park, sx, sy);
        blk = sx[0]; blk_int = sy[0];
    }
    if (GRAD && FLAT) {
        const double gs = nhp_block_sum_n<NW>(gsum, red);
        if (tid == 0) {
            if (ps.direct) ps.grad[c] = gs - a.duration;
            else if (gs != 0.0) atomicAdd(&ps.grad[c], gs);
        }
        __syncthreads();
    }
    NHP_SL_STAMP(3);
    if (!out || defer) {
        if (tid == 0) {
            partials[2 * (size_t)blockIdx.x] = blk;
            partials[2 * (size_t)blockIdx.x + 1] = blk_int;
        }
        NHP_SL_STAMP(4);
        return;
    }
    // fused second stage (as k_windowed): write-through partials, one sharded ticket; the workgroup that draws the last
    // ticket adds all partials in a fixed order and leaves the tickets at 0 for the next launch
    int *flag = reinterpret_cast<int *>(red + 32);
    if (tid == 0) {
        __hip_atomic_store(&partials[2 * (size_t)blockIdx.x], blk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&partials[2 * (size_t)blockIdx.x + 1], blk_int, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int nb = gridDim.x, sh = blockIdx.x % NHP_SL_SHARDS;
        const unsigned int pop = (nb - sh + NHP_SL_SHARDS - 1) / NHP_SL_SHARDS;
        const unsigned int used = nb < NHP_SL_SHARDS ? nb : NHP_SL_SHARDS;
        int last = 0;
        if (__hip_atomic_fetch_add(&counter[32 * (1 + sh)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == pop - 1)
            last = __hip_atomic_fetch_add(&counter[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == used - 1;
        *flag = last;
    }
    __syncthreads();
    NHP_SL_STAMP(4);
    if (!*flag) return;
    double sl_ = 0.0, si = 0.0;
    for (unsigned int i = tid; i < gridDim.x; i += BLOCK) {
        sl_ += __hip_atomic_load(&partials[2 * (size_t)i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        si += __hip_atomic_load(&partials[2 * (size_t)i + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    nhp_block_sum2_n<NW>(sl_, si, red);
    if (tid == 0) *out = (0.0 - si) + sl_;
    for (int i = tid; i <= NHP_SL_SHARDS; i += BLOCK)               // (a one-wave workgroup has 64 threads for the 65 words)
        __hip_atomic_store(&counter[32 * i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- S parameter sets per pass --------------------------------------------------------------------------
// The callers of "log-likelihood evaluations per second" come in batches (the 2P objective calls of a finite-difference
// gradient inside the reference's mle!, src/continuous.jl:190; restarts :200; chain populations).  For S models on one dataset
// a slice's rows are fetched and decoded ONCE; a lane (= child) keeps S running sums, one per model, each term from that
// model's column in LDS (S planes of N + 1 entries).  What a pass then costs is its exponentials: ~18 instructions per pair
// and model + 4 per pair.
#define NHP_SETS_MAX 4
struct nhp_sets {
    const double *p1[NHP_SETS_MAX], *W[NHP_SETS_MAX], *A[NHP_SETS_MAX], *lambda0[NHP_SETS_MAX];
    double *out[NHP_SETS_MAX];
};

// DEFER (S = 2, the paired enqueue route): each model's result must be what k_windowed_slices<BLOCK, C, true,
// false> leaves for it alone, bit for bit, so the integral's terms are formed as there (λ0·T rounded on its own: the single
// kernel's select keeps the compiler from contracting it; every build of this kernel takes the same line) and the sums by the
// shared exit; thread 0 stores the two block sums of model m at index 2·blockIdx.x of ITS result slot's buffer (st.out[m]) and
// k_finalize_slots adds them at the next join: no ticket, no agent-scope atomics.  The integral's partial sums wait in LDS from
// the head on (sl_exit_park): four registers less in the row loop, which is what lets eight waves per SIMD fit (64 VGPRs).
__device__ __forceinline__ double sl_flat_integral(const double lam0, const double duration)
{
#pragma clang fp contract(off)
    return threadIdx.x == 0 ? lam0 * duration : 0.0;
}

template <int BLOCK, int C, int S, bool DEFER = false>
__global__ __launch_bounds__(BLOCK) void k_slices_batch(nhp_cont_args a, nhp_slices sl, nhp_sets st, double *__restrict__ partials,
                                                         unsigned int *__restrict__ counter)
{
    constexpr int NW = BLOCK / 64;
    extern __shared__ __align__(16) unsigned char smem[];
    double *red = reinterpret_cast<double *>(smem);                 // [2 * NW <= 32] + flag at [32]
    double2 *col = reinterpret_cast<double2 *>(smem + 320);         // [S][N + 1]
    double *etab = reinterpret_cast<double *>(col + (size_t)S * (a.N + 1));
    double *park = etab + 64;                                       // the shared exit's sums (sl_exit_bytes(S, NW))
    const int tid = threadIdx.x, lane = tid & 63;
    const double tab_v = nhp_exp2_64[lane];
    const nhp_item it = a.items[blockIdx.x];
    const int c = it.node, N = a.N;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nchild = it.kend - it.kbeg;
    const int s0 = sl.item0[blockIdx.x], ns = sl.item0[blockIdx.x + 1] - s0;
    NHP_SL_STAMP(0);

    typedef sl_chunk<C> chunk;
    uint32_t lane4 = (uint32_t)lane * 4u, lane2 = (uint32_t)lane * 2u;
    auto request = [&](chunk &q, const uint32_t row0, const int r) { sl_request<C>(q, sl.lo, sl.hi, row0, r, lane4, lane2); };
    const sl_ctab rowc = (sl_ctab)sl.row;
    // The head, after k_windowed_slices': the parent nodes in trips of UN·BLOCK, and inside a trip every load -- cnt once per
    // node, then W, θ and (behind a wave-uniform branch) A of G models -- is requested before any is used: one round trip per
    // trip instead of up to three per model and pass.  The first rows of the wave's first slice follow the first trip's requests
    // (their addresses need the slice table only) and arrive while the columns are written to LDS.  UN = 2 for every BLOCK: two
    // models' W, θ, A at 2 nodes a thread are 24 registers, at the single kernel's 4 nodes they would be 48 of the 64 that
    // eight waves per SIMD leave.  The models' table pointers and λ0[m][c] are read once, with the item header: λ0 serves the
    // integral here and the walk below.
    constexpr int UN = 2;
    constexpr int G = S >= 2 ? 2 : 1;                               // models per request group (S = 4: two and two)
    const size_t c0 = (size_t)c * N;                                // column c: wave-uniform bases, the node as a 32-bit offset
    typedef const __attribute__((address_space(1))) double *gptr;   // (global: the pinning below must not leave flat loads)
    gptr Wc[S], Tc[S], Ac[S];
    double lam0[S];
#pragma unroll
    for (int m = 0; m < S; ++m) {
        Wc[m] = (gptr)st.W[m]; Tc[m] = (gptr)st.p1[m]; Ac[m] = (gptr)st.A[m];
        lam0[m] = st.lambda0[m][c];
    }
#pragma unroll
    for (int m = 0; m < S; ++m) asm("" : "+s"(Wc[m]), "+s"(Tc[m]), "+s"(Ac[m]));   // all of them in SGPRs before the first request
    const double unit = __builtin_ldexp(a.dt_max, -sl.dbits);
    const double tlim = sl_term_limit(sl.dbits);
    bool outside = false;
    int j = w;
    uint32_t row0 = 0;
    int K = 0;
    chunk qa, qb;
    double integ[S];
#pragma unroll
    for (int m = 0; m < S; ++m) integ[m] = 0.0;
    // `first`: the item is its node's first, the one that carries the node's integral.  DEFER is launched on all_sole datasets
    // only (nhp_launch_slices_pair refuses others): every item is first, and the kernel knows it when it is compiled; elsewhere
    // it is one wave-uniform branch around the integral's terms.  A model without a mask multiplies by a = 1.0: 1.0·w is w.
    const bool first = DEFER ? true : it.first != 0;
    gptr cntp = (gptr)a.cnt;
    auto at = [](gptr base, const uint32_t off) {                   // a wave-uniform base and the node as a 32-bit BYTE offset
        return *(gptr)((const __attribute__((address_space(1))) char *)base + off);
    };
    for (int p0 = 0; p0 < N; p0 += UN * BLOCK) {
        double cnt_[UN];
        uint32_t off_[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int p = p0 + u * BLOCK + tid;
            off_[u] = (uint32_t)(p < N ? p : 0) * 8u;
            cnt_[u] = first ? at(cntp, off_[u]) : 0.0;
        }
#pragma unroll
        for (int g = 0; g < S; g += G) {
            double w_[G][UN], th_[G][UN], a_[G][UN], wv_[G][UN];
#pragma unroll
            for (int mm = 0; mm < G; ++mm) {
                const int m = g + mm;
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    w_[mm][u] = at(Wc[m] + c0, off_[u]);
                    th_[mm][u] = at(Tc[m] + c0, off_[u]);
                    a_[mm][u] = Ac[m] ? at(Ac[m] + c0, off_[u]) : 1.0;
                }
            }
            if (p0 == 0 && g == 0) {                                 // (N >= 1 on every route that launches this kernel: the first trip always runs)
                if (j < ns) { row0 = rowc[s0 + j]; K = (int)(rowc[s0 + j + 1] - row0); }
                asm volatile("" ::: "memory");
                request(qa, row0, 0);
                asm volatile("" ::: "memory");
            }
#pragma unroll
            for (int mm = 0; mm < G; ++mm) {
                const int m = g + mm;
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    const int p = p0 + u * BLOCK + tid;
                    wv_[mm][u] = a_[mm][u] * w_[mm][u];                // windowed route: the integral is masked too
                    if (p < N) {
                        const double cx = -((th_[mm][u] * unit) * 92.33248261689366);
                        col[(size_t)m * (N + 1) + p] = make_double2(cx, wv_[mm][u] * th_[mm][u]);
                        outside |= sl_term_outside(cx, tlim);
                        if (DEFER) integ[m] += cnt_[u] * wv_[mm][u];   // (the same terms in the same order as below)
                    }
                }
            }
            if (!DEFER && first) {
#pragma unroll
                for (int mm = 0; mm < G; ++mm)
#pragma unroll
                    for (int u = 0; u < UN; ++u)
                        if (p0 + u * BLOCK + tid < N) integ[g + mm] += cnt_[u] * wv_[mm][u];
            }
        }
    }
#pragma unroll
    for (int m = 0; m < S; ++m) {
        if (tid == 0) col[(size_t)m * (N + 1) + N] = make_double2(0.0, 0.0);
        if (first) integ[m] += sl_flat_integral(lam0[m], a.duration);
        sl_exit_park<NW>(integ[m], park, m, w, lane);
    }
    if (tid < 64) etab[tid] = nhp_exp_tab_biased(tab_v, tid);
    sl_limit_post(outside, reinterpret_cast<int *>(red), w, lane);
    __syncthreads();
    NHP_SL_STAMP(1);
    const bool fast = sl_limit_all_inside<NW>(reinterpret_cast<const int *>(red), lane);   // every entry of every model of the pass

    const uint32_t dmask = sl.dmask;
    const int nsh = sl.nsh;
    const nhp_exp_term_consts ekc = nhp_exp_term_setup();
    // (the models' columns stay S planes: interleaved, col[p·S + m], model m sits at a constant offset and a row loses its
    //  v_add_u32, but a ds_read_b128 of one model then finds its 64 nodes on every S-th 16-byte slot only; built, measured and
    //  not taken: DESIGN 3.1d, "The row diet", profiles/r19a_pmc_pair_counters_interleaved.txt)
    const uint32_t plane = (uint32_t)(N + 1) * 16u;                 // bytes between the models' columns
    double prod[S];
    int pexp[S];
#pragma unroll
    for (int m = 0; m < S; ++m) { prod[m] = 1.0; pexp[m] = 0; }
    int rnd = 0;                                                    // the wave's slices in snake order (nhp_slice_of)
    // the walk, once for each path of nhp_exp_term: ONE wave-uniform branch out here, none in the rows
    auto walk = [&](auto fastc) {
        constexpr bool FAST = decltype(fastc)::value;
        auto terms = [&](const uint32_t lo, const uint32_t h, double (&acc)[S]) {
            uint32_t hw;
            asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(hw) : "s"(dmask), "v"(h), "v"(0x43300000u));
            const double v = __hiloint2double((int)hw, (int)lo) - 4503599627370496.0;
            const unsigned char *base = reinterpret_cast<const unsigned char *>(col) + ((h >> nsh) << 4);
#pragma unroll
            for (int m = 0; m < S; ++m) {
                const double2 cw = *reinterpret_cast<const double2 *>(base + m * plane);
                if constexpr (FAST) acc[m] = __builtin_fma(cw.y, nhp_exp_term_fast(cw.x, v, etab, ekc), acc[m]);
                else acc[m] = __builtin_fma(cw.y, nhp_exp_term_slow(cw.x, v, etab, ekc), acc[m]);
            }
        };
        // (the slow path row by row throughout: interleaved, its longer terms would set the kernel's register count)
        auto sum = [&](const chunk &q, const int r, const int K, double (&acc)[S]) {
            if (FAST && r + C <= K) {
#pragma unroll
                for (int u = 0; u < C; ++u) terms(q.lo[u], q.hi[u], acc);
            } else {
#pragma unroll
                for (int u = 0; u < C; ++u)
                    if (r + u < K) terms(q.lo[u], q.hi[u], acc);
            }
        };
        while (j < ns) {
            const int jn = nhp_slice_of(++rnd, w, NW);
            // The next slice's rows from the slice table by a scalar load, requested here and waited for where row0n is first
            // used: no round trip at the top of a slice.  Past the wave's last slice the entry read is the item's last (a
            // valid row for the request below, which nothing sums) and K is not used again.
            const int jc = s0 + (jn < ns ? jn : ns - 1);
            const uint32_t row0n = rowc[jc], rowen = rowc[jc + 1];
            double acc[S];
#pragma unroll
            for (int m = 0; m < S; ++m) acc[m] = 0.0;
            if (K <= 0) request(qa, row0n, 0);
            for (int r0 = 0; r0 < K; r0 += 2 * C) {
                request(qb, row0, r0 + C);
                asm volatile("" ::: "memory");
                sum(qa, r0, K, acc);
                const bool more = r0 + 2 * C < K;
                request(qa, more ? row0 : row0n, more ? r0 + 2 * C : 0);
                asm volatile("" ::: "memory");
                sum(qb, r0 + C, K, acc);
            }
            const int kk = 64 * j + lane;
            if (kk < nchild) {
#pragma unroll
                for (int m = 0; m < S; ++m) {
                    const double lam = lam0[m] + acc[m];
                    prod[m] *= lam < 0.0 ? __builtin_nan("") : __builtin_amdgcn_frexp_mant(lam);
                    pexp[m] += __builtin_amdgcn_frexp_exp(lam);
                }
            }
#pragma unroll
            for (int m = 0; m < S; ++m) {
                pexp[m] += __builtin_amdgcn_frexp_exp(prod[m]);
                prod[m] = __builtin_amdgcn_frexp_mant(prod[m]);
            }
            j = jn; row0 = row0n; K = (int)(rowen - row0n);
        }
    };
    if (fast) walk(std::true_type{}); else walk(std::false_type{});
    NHP_SL_STAMP_WAVE();
    NHP_SL_STAMP(2);
    double sx[S], sy[S];
#pragma unroll
    for (int m = 0; m < S; ++m) { sx[m] = 0.0; sy[m] = 0.0; }
    sl_exit_sums<NW, S>(prod, pexp, park, sx, sy);
    NHP_SL_STAMP(3);
    if (DEFER) {
        if (tid == 0) {
#pragma unroll
            for (int m = 0; m < S; ++m) {
                st.out[m][2 * (size_t)blockIdx.x] = sx[m];
                st.out[m][2 * (size_t)blockIdx.x + 1] = sy[m];
            }
        }
        NHP_SL_STAMP(4);
        return;
    }
    int *flag = reinterpret_cast<int *>(red + 32);
    if (tid == 0) {
#pragma unroll
        for (int m = 0; m < S; ++m) {
            __hip_atomic_store(&partials[(2 * (size_t)blockIdx.x) * S + 2 * m], sx[m], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&partials[(2 * (size_t)blockIdx.x) * S + 2 * m + 1], sy[m], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int nb = gridDim.x, sh = blockIdx.x % NHP_SL_SHARDS;
        const unsigned int pop = (nb - sh + NHP_SL_SHARDS - 1) / NHP_SL_SHARDS;
        const unsigned int used = nb < NHP_SL_SHARDS ? nb : NHP_SL_SHARDS;
        int last = 0;
        if (__hip_atomic_fetch_add(&counter[32 * (1 + sh)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == pop - 1)
            last = __hip_atomic_fetch_add(&counter[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == used - 1;
        *flag = last;
    }
    __syncthreads();
    NHP_SL_STAMP(4);
    if (!*flag) return;
#pragma unroll
    for (int m = 0; m < S; ++m) {
        double sl_ = 0.0, si = 0.0;
        for (unsigned int i = tid; i < gridDim.x; i += BLOCK) {
            sl_ += __hip_atomic_load(&partials[(2 * (size_t)i) * S + 2 * m], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            si += __hip_atomic_load(&partials[(2 * (size_t)i) * S + 2 * m + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        nhp_block_sum2_n<NW>(sl_, si, red);
        if (tid == 0) *st.out[m] = (0.0 - si) + sl_;
        __syncthreads();
    }
    for (int i = tid; i <= NHP_SL_SHARDS; i += BLOCK)
        __hip_atomic_store(&counter[32 * i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- parent sampler over the child slices, logit-normal impulses (config 3's sweep) -------------------------------------
// resample_parent (src/parents.jl:25-46): weights [A·W·ħ(t_i - t_{i-1}), ..., λ0] most recent parent first, their sequential
// sum, one uniform, the first index whose running sum of quotients w_k / s exceeds it.  A child is one lane, as in k_sampler --
// the order of every addition and division is the contract -- but its records arrive row by row from the slice planes (one
// coalesced load per row and wave instead of 64 cache lines per instruction) and the first CACHE weights wait in LDS, row by
// lane, for the scan.  Padding records weigh exactly 0 and are added like the others: x + 0.0 = x, so a child's sum is the
// sequential sum of ITS weights, bit for bit; the scan stops a lane at its own last parent.
__global__ __launch_bounds__(256) void k_slices_build_lq(nhp_cont_args a, nhp_slices sl, double *__restrict__ L, double *__restrict__ Q)
{
#pragma clang fp contract(off)
    const nhp_item it = a.items[blockIdx.x];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nchild = it.kend - it.kbeg;
    const int s0 = sl.item0[blockIdx.x], ns = sl.item0[blockIdx.x + 1] - s0;
    for (int j = w; j < ns; j += 4) {
        const uint32_t row0 = sl.row[s0 + j];
        const int K = (int)(sl.row[s0 + j + 1] - row0);
        const int kk = 64 * j + lane;
        nhp_child ch;
        ch.t = 0.0; ch.first = 0; ch.idx = 0;
        if (kk < nchild) ch = a.child_w[it.kbeg + kk];
        const int len = ch.idx - ch.first;
        for (int r = 0; r < K; ++r) {
            double2 d = make_double2(0.0, 0.0);
            if (r < len) d = nhp_logitnormal_data(a.inv_dtmax, ch.t - a.ev[ch.idx - 1 - r].t);
            const size_t o = ((size_t)row0 + (size_t)r) * 64 + (size_t)lane;
            L[o] = d.x;
            Q[o] = d.y;
        }
    }
}

// Exponential impulses: the sampler's weights are a·w·θ·e^{-θΔt} of the EXACT Δt = t_i - t_j (the slices' 37-bit delay would
// change the low bits of a weight and, once in a long while, the index the scan stops at: the sampler's contract is bit
// equality with the sequential reference).  One more plane, the delays as doubles, made once per dataset like L and Q.
__global__ __launch_bounds__(256) void k_slices_build_d(nhp_cont_args a, nhp_slices sl, double *__restrict__ D)
{
    const nhp_item it = a.items[blockIdx.x];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nchild = it.kend - it.kbeg;
    const int s0 = sl.item0[blockIdx.x], ns = sl.item0[blockIdx.x + 1] - s0;
    for (int j = w; j < ns; j += 4) {
        const uint32_t row0 = sl.row[s0 + j];
        const int K = (int)(sl.row[s0 + j + 1] - row0);
        const int kk = 64 * j + lane;
        nhp_child ch;
        ch.t = 0.0; ch.first = 0; ch.idx = 0;
        if (kk < nchild) ch = a.child_w[it.kbeg + kk];
        const int len = ch.idx - ch.first;
        for (int r = 0; r < K; ++r)
            D[((size_t)row0 + (size_t)r) * 64 + (size_t)lane] = r < len ? ch.t - a.ev[ch.idx - 1 - r].t : 0.0;
    }
}

template <int BLOCK, int CACHE, int IMP>
__global__ __launch_bounds__(BLOCK) void k_sampler_slices(nhp_cont_args a, nhp_slices sl, const double *__restrict__ L, const double *__restrict__ Q,
                                                           const double *__restrict__ u, uint64_t seed, uint64_t step,
                                                           int64_t *__restrict__ parents, int64_t *__restrict__ pnodes,
                                                           int32_t *__restrict__ pn_b, double *__restrict__ dt_b, int *__restrict__ err)
{
#pragma clang fp contract(off)
    constexpr int NW = BLOCK / 64, C = 2;
    extern __shared__ __align__(16) unsigned char smem[];
    double2 *col = reinterpret_cast<double2 *>(smem);               // [N + 1] {μ, √τ}; [N] = {0, 0}
    double *colw = reinterpret_cast<double *>(col + a.N + 1);       // [N + 1] a·w; [N] = 0
    double *cache = colw + a.N + 1;                                 // [NW][CACHE][64] the first weights of the slice's children
    const nhp_item it = a.items[blockIdx.x];
    const int c = it.node, N = a.N, tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nchild = it.kend - it.kbeg;
    const int s0 = sl.item0[blockIdx.x], ns = sl.item0[blockIdx.x + 1] - s0;
    for (int p = tid; p < N; p += BLOCK) {
        const size_t k = (size_t)p + (size_t)c * N;
        double wv = a.W[k];
        if (a.A) wv = a.A[k] * wv;
        if (IMP == NHP_IMPULSE_EXPONENTIAL) {
            // {rate, a·w}: k_sampler<0>'s column.  The rate is inv(scale) of Exponential(1/θ), as the reference and the oracle
            // take it: 1/(1/θ) is not θ for about one double in six, and a weight from θ itself then differs in its last bit
            const double scale = 1.0 / a.p1[k];
            col[p] = make_double2(1.0 / scale, wv);
        } else col[p] = make_double2(a.p1[k], __builtin_sqrt(a.p2[k]));
        colw[p] = wv;
    }
    if (tid == 0) { col[N] = make_double2(0.0, 0.0); colw[N] = 0.0; }
    __syncthreads();
    double *wc = cache + (size_t)w * CACHE * 64 + lane;
    const int nsh = sl.nsh;
    struct chunk { uint32_t hi[C]; double l[C], q[C]; };
    // (exponential: L is the plane of exact delays, Q is not read)
    auto request = [&](chunk &qq, const uint32_t row0, const int r) {
        const size_t o = ((size_t)row0 + (size_t)r) * 64;
#pragma unroll
        for (int x = 0; x < C; ++x) {
            qq.hi[x] = sl.hi[o + x * 64 + lane];
            qq.l[x] = L[o + x * 64 + lane];
            qq.q[x] = IMP == NHP_IMPULSE_EXPONENTIAL ? 0.0 : Q[o + x * 64 + lane];
        }
    };
    auto weight = [&](const uint32_t h, const double l, const double q) {
        const int p = (int)(h >> nsh);
        const double2 cq = col[p];
        if (IMP == NHP_IMPULSE_EXPONENTIAL) return cq.y * nhp_pdf_exponential(cq.x, l);   // the operations of samp_weight<0>
        return colw[p] * nhp_pdf_logitnormal_cached(cq.x, cq.y, make_double2(l, q));
    };
    for (int j = w; j < ns; j += NW) {
        const uint32_t row0 = sl.row[s0 + j];
        const int K = (int)(sl.row[s0 + j + 1] - row0);
        const int kk = 64 * j + lane;
        const bool valid = kk < nchild;
        nhp_child ch;
        ch.t = 0.0; ch.first = 0; ch.idx = 0;
        if (valid) ch = a.child_w[it.kbeg + kk];
        const int i = ch.idx, nreal = ch.idx - ch.first, n = nreal + 1;
        const double t = ch.t;
        const double base = valid ? sl_baseline(a, c, t) : 1.0;
        // ---- the sum, most recent parent first (0 + w_0 = w_0; the padding rows add 0), the baseline last
        double v = 0.0;
        chunk qa, qb;
        request(qa, row0, 0);
        for (int r0 = 0; r0 < K; r0 += 2 * C) {
            request(qb, row0, r0 + C);
            asm volatile("" ::: "memory");
#pragma unroll
            for (int x = 0; x < C; ++x)
                if (r0 + x < K) {
                    const double wk = weight(qa.hi[x], qa.l[x], qa.q[x]);
                    if (r0 + x < CACHE) wc[(size_t)(r0 + x) * 64] = wk;
                    v = v + wk;
                }
            request(qa, row0, r0 + 2 * C);
            asm volatile("" ::: "memory");
#pragma unroll
            for (int x = 0; x < C; ++x)
                if (r0 + C + x < K) {
                    const double wk = weight(qb.hi[x], qb.l[x], qb.q[x]);
                    if (r0 + C + x < CACHE) wc[(size_t)(r0 + C + x) * 64] = wk;
                    v = v + wk;
                }
        }
        const double s = v + base;
        const bool live = valid && i > 0;                           // index == 1 -> (0, 0): src/parents.jl:26-28
        if (live && (!(s > 0.0) || !(s < __builtin_inf()))) *err = 1;
        const double draw = live ? (u ? u[i] : nhp_philox_uniform(seed, step, (uint64_t)i)) : 0.0;
        // ---- the scan: cp_k = cp_{k-1} + w_k / s while cp_k <= u and k < n - 1 (the lanes of the wave step together; a lane
        //      that has stopped stays stopped).  Weight k of a child: its k-th parent, or the baseline at k = n - 1.
        auto wk_at = [&](const int k) {
            if (k >= nreal) return base;
            if (k < CACHE) return wc[(size_t)k * 64];
            const size_t o = ((size_t)row0 + (size_t)k) * 64 + lane;
            return weight(sl.hi[o], L[o], IMP == NHP_IMPULSE_EXPONENTIAL ? 0.0 : Q[o]);
        };
        int kk2 = 0;
        double cp = live ? wk_at(0) / s : 0.0;
        bool go = live && cp <= draw && kk2 < n - 1;
        while (__ballot(go)) {
            if (go) {
                ++kk2;
                cp = cp + wk_at(kk2) / s;
                go = cp <= draw && kk2 < n - 1;
            }
        }
        if (valid) {
            const int parent = (live && kk2 < n - 1) ? i - 1 - kk2 : -1;
            const int pnode = parent >= 0 ? a.nodes[parent] : -1;
            if (parents) parents[i] = (int64_t)parent + 1;          // 1-based event index, 0 = baseline
            if (pnodes) pnodes[i] = (int64_t)pnode + 1;
            const int kb = a.wpos[it.kbeg + kk];
            pn_b[kb] = pnode;
            dt_b[kb] = parent >= 0 ? t - a.times[parent] : 0.0;
        }
    }
}

// ---- logit-normal impulses over the child slices: log-likelihood -------------------------------------------------------------
// The same walk as k_windowed_slices -- one lane per child, rows of 64 records, most recent parent first -- with the record's
// node from the `hi` plane and the data half of its pdf, {logit(x), 1/(x(1-x))}, from the planes the parent sampler keeps
// (sl_L, sl_Q: k_slices_build_lq), the column {μ, √τ} and a·w in LDS: a term is a·w · nhp_pdf_logitnormal_cached, the pair
// cache's arithmetic.  A separate kernel so that the exponential one's code is not touched.
template <int BLOCK, int C, bool FLAT>
__global__ __launch_bounds__(BLOCK) void k_windowed_slices_ln(nhp_cont_args a, nhp_slices sl, const double *__restrict__ L, const double *__restrict__ Q,
                                                               int mask_integral, double *__restrict__ partials, unsigned int *__restrict__ counter,
                                                               double *__restrict__ out, double *__restrict__ lambda_out, int defer)
{
    constexpr int NW = BLOCK / 64;
    extern __shared__ __align__(16) unsigned char smem[];
    double *red = reinterpret_cast<double *>(smem);                 // [2 * NW <= 32] + flag at [32]
    double2 *col = reinterpret_cast<double2 *>(smem + 320);         // [N + 1] {μ, √τ}; [N] = {0, 0}
    double *colw = reinterpret_cast<double *>(col + a.N + 1);       // [N + 1] a·w; [N] = 0
    const int tid = threadIdx.x, lane = tid & 63;
    const nhp_item it = a.items[blockIdx.x];
    const int c = it.node, N = a.N;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nchild = it.kend - it.kbeg;
    const int s0 = sl.item0[blockIdx.x], ns = sl.item0[blockIdx.x + 1] - s0;
    struct chunk { uint32_t hi[C]; double l[C], q[C]; };
    auto request = [&](chunk &qq, const uint32_t row0, const int r) {
        const size_t o = ((size_t)row0 + (size_t)r) * 64;
#pragma unroll
        for (int u = 0; u < C; ++u) {
            qq.hi[u] = sl.hi[o + u * 64 + lane];
            qq.l[u] = L[o + u * 64 + lane];
            qq.q[u] = Q[o + u * 64 + lane];
        }
    };
    int j = w;
    uint32_t row0 = 0;
    int K = 0;
    chunk qa, qb;
    double integ = 0.0;
    for (int p0 = 0; p0 < N; p0 += BLOCK) {
        const int p = p0 + tid;
        const size_t k = (size_t)(p < N ? p : 0) + (size_t)c * N;
        const double w_ = a.W[k], mu = a.p1[k], tau = a.p2[k], a_ = a.A ? a.A[k] : 1.0, cnt_ = it.first ? a.cnt[p < N ? p : 0] : 0.0;
        if (p0 == 0) {
            if (j < ns) { row0 = sl.row[s0 + j]; K = (int)(sl.row[s0 + j + 1] - row0); }
            asm volatile("" ::: "memory");
            request(qa, row0, 0);
            asm volatile("" ::: "memory");
        }
        if (p < N) {
            double wv = w_, wint = w_;
            if (a.A) { wv = a_ * wv; if (mask_integral) wint = wv; }
            col[p] = make_double2(mu, __builtin_sqrt(tau));
            colw[p] = wv;
            integ += cnt_ * wint;
        }
    }
    if (tid == 0) { col[N] = make_double2(0.0, 0.0); colw[N] = 0.0; }
    if (out && it.first) integ += sl_baseline_integral_col(a, c);
    __syncthreads();
    const double lam0 = FLAT ? a.lambda0[c] : 0.0;
    const int nsh = sl.nsh;
    auto term = [&](const uint32_t h, const double l, const double q) {
        const int p = (int)(h >> nsh);
        const double2 cq = col[p];
        return colw[p] * nhp_pdf_logitnormal_cached(cq.x, cq.y, make_double2(l, q));
    };
    auto sum = [&](const chunk &qq, const int r, const int K, double s) {
        if (r + C <= K) {
            double t[C];
#pragma unroll
            for (int u = 0; u < C; ++u) t[u] = term(qq.hi[u], qq.l[u], qq.q[u]);
#pragma unroll
            for (int u = 0; u < C; ++u) s += t[u];
        } else {
#pragma unroll
            for (int u = 0; u < C; ++u)
                if (r + u < K) s += term(qq.hi[u], qq.l[u], qq.q[u]);
        }
        return s;
    };
    double prod = 1.0;
    int pexp = 0;
    int rnd = 0;                                                    // the wave's slices in snake order (nhp_slice_of)
    while (j < ns) {
        const int jn = nhp_slice_of(++rnd, w, NW);
        uint32_t row0n = 0;
        int Kn = 0;
        if (jn < ns) { row0n = sl.row[s0 + jn]; Kn = (int)(sl.row[s0 + jn + 1] - row0n); }
        double s = 0.0;
        if (K <= 0) request(qa, row0n, 0);
        for (int r0 = 0; r0 < K; r0 += 2 * C) {
            request(qb, row0, r0 + C);
            asm volatile("" ::: "memory");
            s = sum(qa, r0, K, s);
            const bool more = r0 + 2 * C < K;
            request(qa, more ? row0 : row0n, more ? r0 + 2 * C : 0);
            asm volatile("" ::: "memory");
            s = sum(qb, r0 + C, K, s);
        }
        const int kk = 64 * j + lane;
        if (kk < nchild) {
            const double tk = FLAT ? 0.0 : a.child_w[it.kbeg + kk].t;
            const double lam = (FLAT ? lam0 : sl_baseline(a, c, tk)) + s;
            prod *= lam < 0.0 ? __builtin_nan("") : __builtin_amdgcn_frexp_mant(lam);
            pexp += __builtin_amdgcn_frexp_exp(lam);
            if (lambda_out) lambda_out[a.child_w[it.kbeg + kk].idx] = lam;           // (total_intensity, the two-pass gradient's 1/λ)
        }
        pexp += __builtin_amdgcn_frexp_exp(prod);
        prod = __builtin_amdgcn_frexp_mant(prod);
        j = jn; row0 = row0n; K = Kn;
    }
    double acc = nhp_log(prod) + (double)pexp * 6.93147180559945286e-01;
    if (prod == 0.0) acc = -__builtin_inf();
    double blk = acc, blk_int = integ;
    nhp_block_sum2_n<NW>(blk, blk_int, red);
    if (!out || defer) {                                            // (defer: as in k_windowed_slices)
        if (tid == 0) { partials[2 * (size_t)blockIdx.x] = blk; partials[2 * (size_t)blockIdx.x + 1] = blk_int; }
        return;
    }
    int *flag = reinterpret_cast<int *>(red + 32);                  // the fused second stage of k_windowed_slices
    if (tid == 0) {
        __hip_atomic_store(&partials[2 * (size_t)blockIdx.x], blk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&partials[2 * (size_t)blockIdx.x + 1], blk_int, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int nb = gridDim.x, sh = blockIdx.x % NHP_SL_SHARDS;
        const unsigned int pop = (nb - sh + NHP_SL_SHARDS - 1) / NHP_SL_SHARDS;
        const unsigned int used = nb < NHP_SL_SHARDS ? nb : NHP_SL_SHARDS;
        int last = 0;
        if (__hip_atomic_fetch_add(&counter[32 * (1 + sh)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == pop - 1)
            last = __hip_atomic_fetch_add(&counter[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == used - 1;
        *flag = last;
    }
    __syncthreads();
    if (!*flag) return;
    double sl_ = 0.0, si = 0.0;
    for (unsigned int i = tid; i < gridDim.x; i += BLOCK) {
        sl_ += __hip_atomic_load(&partials[2 * (size_t)i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        si += __hip_atomic_load(&partials[2 * (size_t)i + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    nhp_block_sum2_n<NW>(sl_, si, red);
    if (tid == 0) *out = (0.0 - si) + sl_;
    for (int i = tid; i <= NHP_SL_SHARDS; i += BLOCK)
        __hip_atomic_store(&counter[32 * i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static nhp_slices slices_view(const nhp_cont_dataset *ds)
{
    nhp_slices sl;
    sl.row = ds->d_sl_row; sl.item0 = ds->d_sl_item0; sl.lo = ds->d_sl_lo; sl.hi = ds->d_sl_hi;
    sl.nsh = 16 - ds->sl_nb;
    sl.dmask = (1u << sl.nsh) - 1u;
    sl.dbits = 32 + sl.nsh;
    return sl;
}

// the planes, made at the first evaluation that wants them (data only)
static nhp_status ensure_slices(nhp_ctx *ctx, const nhp_cont_dataset *cds, const nhp_cont_args &a)
{
    if (cds->d_sl_lo) return NHP_OK;
    nhp_cont_dataset *ds = const_cast<nhp_cont_dataset *>(cds);
    const size_t n = ((size_t)ds->sl_rows + 16) * 64;
    if (hipMalloc((void **)&ds->d_sl_lo, 4 * n) != hipSuccess || hipMalloc((void **)&ds->d_sl_hi, 2 * n) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(ds->d_sl_lo); (void)hipFree(ds->d_sl_hi);
        ds->d_sl_lo = nullptr; ds->d_sl_hi = nullptr;
        nhp_set_error(ctx, "out of device memory (child slices)");
        return NHP_ENOMEM;
    }
    NHP_HIP(ctx, hipMemsetAsync(ds->d_sl_lo + (size_t)ds->sl_rows * 64, 0, 4 * 16 * 64, ctx->main()));
    NHP_HIP(ctx, hipMemsetAsync(ds->d_sl_hi + (size_t)ds->sl_rows * 64, 0, 2 * 16 * 64, ctx->main()));
    const nhp_slices sl = slices_view(ds);
    if (ds->n_items > 0)
        hipLaunchKernelGGL(k_slices_build, dim3((unsigned)ds->n_items), dim3(256), 0, ctx->main(), a, sl, ds->d_sl_lo, ds->d_sl_hi);
    NHP_HIP(ctx, hipGetLastError());
    return NHP_OK;
}

static nhp_pslices pslices_view(const nhp_cont_dataset *ds)
{
    nhp_pslices ps;
    ps.row = ds->d_ps_row; ps.perm = ds->d_ps_perm; ps.lo = ds->d_ps_lo; ps.hi = ds->d_ps_hi;
    ps.spi = ds->ps_spi;
    ps.psh = 16 - ds->ps_sb;
    ps.dmask = (1u << ps.psh) - 1u;
    ps.dbits = 32 + ps.psh;
    ps.max_item = ds->max_item;
    ps.direct = 0;
    ps.grad = nullptr;
    return ps;
}

// The parent slices, made at the first gradient that wants them (data only): pair counts by (item, parent node) -> the
// lanes' order and every slice's rows (device) -> row offsets (host prefix sum over n_items·spi numbers: the one
// synchronisation) -> fill through LDS tickets -> every lane sorted.
static nhp_status ensure_parent_slices(nhp_ctx *ctx, const nhp_cont_dataset *cds, const nhp_cont_args &a)
{
    if (cds->d_ps_lo) return NHP_OK;
    nhp_cont_dataset *ds = const_cast<nhp_cont_dataset *>(cds);
    const int N = ds->N, spi = (N + 63) / 64, ni = ds->n_items;
    int sb = 0;
    while (((int64_t)1 << sb) <= ds->max_item) ++sb;               // bit length of max_item: the padding records' slot
    if (sb > 16 || 4 * (size_t)N > 160 * 1024) { nhp_set_error(ctx, "parent slices: item or node count out of range"); return NHP_ENOTIMPL; }
    uint32_t *d_cnt = nullptr, *d_rows = nullptr;
    uint16_t *d_rankof = nullptr;
    auto fail = [&](nhp_status st, const char *what) {
        (void)hipGetLastError();
        (void)hipFree(d_cnt); (void)hipFree(d_rows); (void)hipFree(d_rankof);
        (void)hipFree(ds->d_ps_row); (void)hipFree(ds->d_ps_perm); (void)hipFree(ds->d_ps_lo); (void)hipFree(ds->d_ps_hi);
        ds->d_ps_row = nullptr; ds->d_ps_perm = nullptr; ds->d_ps_lo = nullptr; ds->d_ps_hi = nullptr;
        nhp_set_error(ctx, "parent slices: %s", what);
        return st;
    };
    if (hipMalloc((void **)&d_cnt, 4 * (size_t)ni * N) != hipSuccess || hipMalloc((void **)&d_rows, 4 * (size_t)ni * spi) != hipSuccess ||
        hipMalloc((void **)&d_rankof, 2 * (size_t)ni * N) != hipSuccess ||
        hipMalloc((void **)&ds->d_ps_perm, 2 * (size_t)ni * spi * 64) != hipSuccess ||
        hipMalloc((void **)&ds->d_ps_row, 4 * ((size_t)ni * spi + 1)) != hipSuccess)
        return fail(NHP_ENOMEM, "out of device memory");
    const size_t lds = 4 * (size_t)N;
    if (lds > 64 * 1024) {
        (void)hipFuncSetAttribute((const void *)k_ps_count, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        (void)hipFuncSetAttribute((const void *)k_ps_rank, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        (void)hipFuncSetAttribute((const void *)k_ps_fill, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }
    hipLaunchKernelGGL(k_ps_count, dim3((unsigned)ni), dim3(256), lds, ctx->main(), a, d_cnt);
    hipLaunchKernelGGL(k_ps_rank, dim3((unsigned)ni), dim3(256), lds, ctx->main(), N, spi, d_cnt, ds->d_ps_perm, d_rankof, d_rows);
    if (hipGetLastError() != hipSuccess) return fail(NHP_EHIP, "launch failed");
    std::vector<uint32_t> rows((size_t)ni * spi), off((size_t)ni * spi + 1);
    if (hipMemcpyAsync(rows.data(), d_rows, 4 * rows.size(), hipMemcpyDeviceToHost, ctx->main()) != hipSuccess ||
        hipStreamSynchronize(ctx->main()) != hipSuccess) return fail(NHP_EHIP, "copy failed");
    uint64_t run = 0;
    for (size_t q = 0; q < rows.size(); ++q) { off[q] = (uint32_t)run; run += rows[q]; }
    off[rows.size()] = (uint32_t)run;
    if (run >= ((uint64_t)1 << 25)) return fail(NHP_ENOTIMPL, "too many rows");
    ds->ps_rows = (int64_t)run; ds->ps_spi = spi; ds->ps_sb = sb;
    const size_t n = ((size_t)run + 16) * 64;
    if (hipMalloc((void **)&ds->d_ps_lo, 4 * n) != hipSuccess || hipMalloc((void **)&ds->d_ps_hi, 2 * n) != hipSuccess)
        return fail(NHP_ENOMEM, "out of device memory");
    if (hipMemcpyAsync(ds->d_ps_row, off.data(), 4 * off.size(), hipMemcpyHostToDevice, ctx->main()) != hipSuccess ||
        hipMemsetAsync(ds->d_ps_lo + (size_t)run * 64, 0, 4 * 16 * 64, ctx->main()) != hipSuccess ||
        hipMemsetAsync(ds->d_ps_hi + (size_t)run * 64, 0, 2 * 16 * 64, ctx->main()) != hipSuccess)
        return fail(NHP_EHIP, "copy failed");
    const nhp_pslices ps = pslices_view(ds);
    hipLaunchKernelGGL(k_ps_fill, dim3((unsigned)ni), dim3(256), lds, ctx->main(), a, ps, d_cnt, d_rankof, ds->d_ps_lo, ds->d_ps_hi);
    hipLaunchKernelGGL(k_ps_sort, dim3((unsigned)ni), dim3(256), 0, ctx->main(), N, ps, d_cnt, ds->d_ps_lo, ds->d_ps_hi);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->main()) != hipSuccess) return fail(NHP_EHIP, "fill failed");   // (`off` and the scratch go out of scope)
    (void)hipFree(d_cnt); (void)hipFree(d_rows); (void)hipFree(d_rankof);
    return NHP_OK;
}

// the workgroup size and the rows per request of k_windowed_slices on this dataset (the paired launch takes the same)
static void slices_cfg(const nhp_cont_dataset *ds, int *B, int *C)
{
    const int per_item = (ds->max_item + 63) / 64;
    // (rows in flight per wave = 2C: short slices are served by L2 / the Infinity Cache and want few, long ones stream from HBM)
    const double mean_rows = ds->n_slices > 0 ? (double)ds->sl_rows / (double)ds->n_slices : 0.0;
    *B = per_item >= 12 ? 512 : per_item >= 6 ? 256 : per_item >= 3 ? 128 : 64;
    *C = mean_rows >= 48.0 ? 8 : mean_rows >= 16.0 ? 4 : 2;
    if (const char *cfg = getenv("NHP_SLICES_CFG")) sscanf(cfg, "%d,%d", B, C);
}

// grad != nullptr: log-likelihood AND gradient (k_windowed_slices<.., GRAD>); the gradient must have been initialised by
// k_grad_init unless `direct`
static nhp_status launch_slices(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, int mask_integral, double *d_out,
                                double *d_grad, bool direct, bool *launched, int32_t defer_slot = -1, bool *deferred = nullptr)
{
    *launched = false;
    if (deferred) *deferred = false;
    if (!ds->d_sl_row || ds->n_items <= 0 || m->impulse_kind != NHP_IMPULSE_EXPONENTIAL) return NHP_OK;
    if (nhp_slices_off(d_grad ? "NHP_GRAD_SLICES" : nullptr)) return NHP_OK;     // (NHP_GRAD_SLICES=0: the two-pass route of cont_grad.hip)
    // waves per workgroup from the slices an item has (one item per node at N >= 1024: ~15 slices; short items at small N);
    // rows per request from the windows' length.  NHP_SLICES_CFG = "BLOCK,C" overrides (tools/dbg/slicesweep.sh)
    int B, C;
    slices_cfg(ds, &B, &C);
    if (!((B == 64 || B == 128 || B == 256 || B == 512 || B == 1024) && (C == 2 || C == 4 || C == 8))) { B = 256; C = 4; }
    // (behind the column and the 2^(j/64) table: the gradient's 1/λ, or the shared exit's sums for the waves of this launch)
    const size_t lds = d_grad ? 320 + 16 * ((size_t)ds->N + 1) + 512 + 8 * ((size_t)ds->max_item + 1) : sl_lds_bytes(ds->N, 1, B);
    if (lds > 160 * 1024) return NHP_OK;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_ctx_reserve_partials(ctx, 2 * (size_t)ds->n_items));
    nhp_cont_args a = nhp_make_args(ds, m);
    NHP_TRY(ensure_slices(ctx, ds, a));
    const nhp_slices sl = slices_view(ds);
    nhp_pslices ps{};
    if (d_grad) {
        NHP_TRY(ensure_parent_slices(ctx, ds, a));
        ps = pslices_view(ds);
        ps.grad = d_grad;
        ps.direct = direct ? 1 : 0;
    }
    dim3 grid((unsigned)ds->n_items);
    bool ok = false;
    const bool flat = m->baseline_kind == NHP_BASELINE_HOMOGENEOUS;
    // the enqueue route: the block sums into the slot's own buffer, added up at the next join (k_finalize_slots repeats the
    // order of a workgroup of up to 512; one of 1024 keeps its fused sum)
    const bool known = (B == 64 || B == 128 || B == 256 || B == 512) && (C == 2 || C == 4 || C == 8);
    const int defer = defer_slot >= 0 && !d_grad && d_out && known ? 1 : 0;
    double *partials = ctx->d_partials;
    if (defer) {
        NHP_TRY(nhp_ctx_reserve_slot_partials(ctx, defer_slot, 2 * (size_t)ds->n_items));
        partials = ctx->d_slot_partials[defer_slot];
    }
#define NHP_SLAUNCH(b, cc, f, g)                                                                                      \
    do {                                                                                                              \
        if (lds > 64 * 1024)                                                                                          \
            (void)hipFuncSetAttribute((const void *)k_windowed_slices<b, cc, f, g>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        hipLaunchKernelGGL((k_windowed_slices<b, cc, f, g>), grid, dim3(b), lds, ctx->lane(), a, sl, ps, mask_integral, partials, \
                           ctx->d_counter, d_out, defer);                                                             \
    } while (0)
#define NHP_SCASE(b, cc)                                                                                              \
    if (!ok && B == b && C == cc) {                                                                                   \
        ok = true;                                                                                                    \
        if (d_grad) { if (flat) NHP_SLAUNCH(b, cc, true, true); else NHP_SLAUNCH(b, cc, false, true); }               \
        else { if (flat) NHP_SLAUNCH(b, cc, true, false); else NHP_SLAUNCH(b, cc, false, false); }                    \
    }
#define NHP_SROW(b) NHP_SCASE(b, 2) NHP_SCASE(b, 4) NHP_SCASE(b, 8)
    NHP_SROW(64) NHP_SROW(128) NHP_SROW(256) NHP_SROW(512) NHP_SROW(1024)
#undef NHP_SLAUNCH
#undef NHP_SROW
#undef NHP_SCASE
    NHP_HIP(ctx, hipGetLastError());
    if (defer) {
        ctx->pend.mark(defer_slot, ds->n_items, B);
        if (deferred) *deferred = true;
    }
    *launched = true;
    return NHP_OK;
}

nhp_status nhp_launch_windowed_slices(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, int mask_integral,
                                      double *d_out, bool *launched, int32_t defer_slot, bool *deferred)
{
    return launch_slices(ctx, ds, m, mask_integral, d_out, nullptr, false, launched, defer_slot, deferred);
}

static nhp_status ensure_lq_planes(nhp_ctx *ctx, nhp_cont_dataset *ds, const nhp_cont_args &a, const nhp_slices &sl, bool *ok);

// logit-normal impulses: the same call for k_windowed_slices_ln (NHP_SLICES_LN=0: the pair-cache kernel)
nhp_status nhp_launch_windowed_slices_ln(nhp_ctx *ctx, const nhp_cont_dataset *cds, const nhp_cont_model *m, int mask_integral,
                                         double *d_out, double *d_lambda, bool *launched, int32_t defer_slot, bool *deferred)
{
    *launched = false;
    if (deferred) *deferred = false;
    if (!cds->d_sl_row || cds->n_items <= 0 || m->impulse_kind != NHP_IMPULSE_LOGITNORMAL) return NHP_OK;
    if (nhp_slices_off("NHP_SLICES_LN")) return NHP_OK;
    const size_t lds = 320 + 24 * ((size_t)cds->N + 1);
    if (lds > 160 * 1024) return NHP_OK;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_ctx_reserve_partials(ctx, 2 * (size_t)cds->n_items));
    nhp_cont_args a = nhp_make_args(cds, m);
    NHP_TRY(ensure_slices(ctx, cds, a));
    nhp_cont_dataset *ds = const_cast<nhp_cont_dataset *>(cds);
    const nhp_slices sl = slices_view(ds);
    bool planes = false;
    NHP_TRY(ensure_lq_planes(ctx, ds, a, sl, &planes));
    if (!planes) return NHP_OK;
    const int per_item = (ds->max_item + 63) / 64;
    const double mean_rows = ds->n_slices > 0 ? (double)ds->sl_rows / (double)ds->n_slices : 0.0;
    // (metric size, µs per evaluation: 512 threads x 2 rows 35.2, 512 x 4 37.0, 256 x 2 34.3, 256 x 4 36.8, 64 x 2 48.9; the pair cache 39.5)
    int B = per_item >= 3 ? 256 : 64, C = mean_rows >= 32.0 ? 4 : 2;
    if (const char *cfg = getenv("NHP_SLICES_LN_CFG")) sscanf(cfg, "%d,%d", &B, &C);
    if (!((B == 64 || B == 256 || B == 512) && (C == 2 || C == 4))) { B = 256; C = 2; }
    const bool flat = m->baseline_kind == NHP_BASELINE_HOMOGENEOUS;
    dim3 grid((unsigned)ds->n_items);
    const int defer = defer_slot >= 0 && d_out && !d_lambda ? 1 : 0;     // (as launch_slices; every workgroup size here is <= 512)
    double *partials = ctx->d_partials;
    if (defer) {
        NHP_TRY(nhp_ctx_reserve_slot_partials(ctx, defer_slot, 2 * (size_t)ds->n_items));
        partials = ctx->d_slot_partials[defer_slot];
    }
#define NHP_LNL(b, cc, f)                                                                                             \
    do {                                                                                                              \
        if (lds > 64 * 1024)                                                                                          \
            (void)hipFuncSetAttribute((const void *)k_windowed_slices_ln<b, cc, f>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        hipLaunchKernelGGL((k_windowed_slices_ln<b, cc, f>), grid, dim3(b), lds, ctx->lane(), a, sl, (const double *)ds->d_sl_L,  \
                           (const double *)ds->d_sl_Q, mask_integral, partials, ctx->d_counter, d_out, d_lambda, defer); \
    } while (0)
#define NHP_LNC(b, cc) do { if (flat) NHP_LNL(b, cc, true); else NHP_LNL(b, cc, false); } while (0)
    if (B == 64) { if (C == 2) NHP_LNC(64, 2); else NHP_LNC(64, 4); }
    else if (B == 256) { if (C == 2) NHP_LNC(256, 2); else NHP_LNC(256, 4); }
    else { if (C == 2) NHP_LNC(512, 2); else NHP_LNC(512, 4); }
#undef NHP_LNC
#undef NHP_LNL
    NHP_HIP(ctx, hipGetLastError());
    if (defer) {
        ctx->pend.mark(defer_slot, ds->n_items, B);
        if (deferred) *deferred = true;
    }
    *launched = true;
    return NHP_OK;
}

// Log-likelihood -> *d_out and gradient -> d_grad [P] of the dataset's own windows (mask_integral = 1: the windowed route's
// masked integral).  When every item is its node's only one, the dataset is whole and the baseline flat, the kernel stores
// every entry of the gradient itself; otherwise k_grad_init (cont_grad.hip) must have run on d_grad (*needs_init).
nhp_status nhp_launch_grad_slices(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, double *d_out, double *d_grad,
                                  bool *launched)
{
    *launched = false;
    ctx->join_lanes();                                  // (launch_slices takes the lane's raw stream: the gradient joins first)
    const bool direct = ds->all_sole && !nhp_is_column_shard(ds) && m->baseline_kind == NHP_BASELINE_HOMOGENEOUS;
    return launch_slices(ctx, ds, m, 1, d_out, d_grad, direct, launched);
}

bool nhp_grad_slices_direct(const nhp_cont_dataset *ds, const nhp_cont_model *m)
{
    return ds->all_sole && !nhp_is_column_shard(ds) && m->baseline_kind == NHP_BASELINE_HOMOGENEOUS;
}

// diagnostics (tools/dbg): the parent-slice planes as they sit on the device; returns the number of records (rows * 64), or -1
extern "C" int64_t nhp_debug_parent_slices(const nhp_cont_dataset *ds, uint32_t *lo, uint16_t *hi, int64_t cap)
{
    if (!ds || !ds->d_ps_lo) return -1;
    const int64_t n = ds->ps_rows * 64;
    if (lo && hi && cap >= n) {
        if (hipMemcpy(lo, ds->d_ps_lo, 4 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return -2;
        if (hipMemcpy(hi, ds->d_ps_hi, 2 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return -2;
    }
    return n;
}

// the workgroup size and the rows per request of the fused k_slices_batch on this dataset
// (the columns of S models leave room for two workgroups of 512 per CU at N = 1024, S = 4; NHP_SETS_CFG = "BLOCK,C" overrides)
static void sets_cfg(const nhp_cont_dataset *ds, int *B, int *C)
{
    const double mean_rows = ds->n_slices > 0 ? (double)ds->sl_rows / (double)ds->n_slices : 0.0;
    *B = (ds->max_item + 63) / 64 >= 6 ? 512 : 256;
    *C = mean_rows >= 16.0 ? 4 : 2;
    if (const char *cfg = getenv("NHP_SETS_CFG")) sscanf(cfg, "%d,%d", B, C);
    if (*B != 256 && *B != 1024) *B = 512;
    if (*C != 2) *C = 4;
}

template <int S>
static nhp_status launch_sets(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *const *ms, int32_t slot0, int B, int C, size_t lds)
{
    NHP_TRY(nhp_ctx_reserve_partials(ctx, 2 * (size_t)ds->n_items * S));
    nhp_cont_args a = nhp_make_args(ds, ms[0]);
    NHP_TRY(ensure_slices(ctx, ds, a));
    const nhp_slices sl = slices_view(ds);
    nhp_sets st;
    for (int k = 0; k < NHP_SETS_MAX; ++k) {
        const nhp_cont_model *m = ms[k < S ? k : 0];
        st.p1[k] = m->d_p1; st.W[k] = m->d_W; st.A[k] = m->has_A ? m->d_A : nullptr; st.lambda0[k] = m->d_lambda0;
        st.out[k] = ctx->d_results + slot0 + (k < S ? k : 0);
    }
    dim3 grid((unsigned)ds->n_items);
#define NHP_BL(b, cc)                                                                                                  \
    do {                                                                                                               \
        if (lds > 64 * 1024)                                                                                           \
            (void)hipFuncSetAttribute((const void *)k_slices_batch<b, cc, S>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        hipLaunchKernelGGL((k_slices_batch<b, cc, S>), grid, dim3(b), lds, ctx->lane(), a, sl, st, ctx->d_partials, ctx->d_counter); \
    } while (0)
    if (B == 256 && C == 2) NHP_BL(256, 2); else if (B == 256) NHP_BL(256, 4);
    else if (B == 1024 && C == 2) NHP_BL(1024, 2); else if (B == 1024) NHP_BL(1024, 4);
    else if (C == 2) NHP_BL(512, 2); else NHP_BL(512, 4);
#undef NHP_BL
    NHP_HIP(ctx, hipGetLastError());
    return NHP_OK;
}

nhp_status nhp_launch_slices_batch(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *const *ms, int S, int32_t slot0,
                                   bool *launched)
{
    *launched = false;
    if (!ds->d_sl_row || ds->n_items <= 0 || (S != 2 && S != 4)) return NHP_OK;
    if (nhp_slices_off("NHP_BATCH_SLICES")) return NHP_OK;
    for (int k = 0; k < S; ++k)
        if (!ms[k] || ms[k]->impulse_kind != NHP_IMPULSE_EXPONENTIAL || ms[k]->baseline_kind != NHP_BASELINE_HOMOGENEOUS) return NHP_OK;
    int B, C;
    sets_cfg(ds, &B, &C);
    const size_t lds = sl_lds_bytes(ds->N, S, B);
    if (lds > 160 * 1024) return NHP_OK;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    if (S == 4) NHP_TRY(launch_sets<4>(ctx, ds, ms, slot0, B, C, lds)); else NHP_TRY(launch_sets<2>(ctx, ds, ms, slot0, B, C, lds));
    *launched = true;
    return NHP_OK;
}

// ---- two enqueued evaluations in one pass ----------------------------------------------------------------------
// Whether an enqueue of (ds, m) would take k_windowed_slices' deferred exit AND may share a pass: exponential impulses, flat
// baseline, one item per node on a whole dataset, a workgroup of at most 512, and two columns in LDS four times per CU.
bool nhp_slices_pair_eligible(const nhp_cont_dataset *ds, const nhp_cont_model *m)
{
    if (!ds || !m || !ds->d_sl_row || ds->n_items <= 0) return false;
    if (m->impulse_kind != NHP_IMPULSE_EXPONENTIAL || m->baseline_kind != NHP_BASELINE_HOMOGENEOUS) return false;
    if (!ds->all_sole || nhp_is_column_shard(ds) || nhp_slices_off(nullptr)) return false;
    if (const char *pl = getenv("NHP_PLIST")) if (atoi(pl) == 0) return false;
    int B, C;
    slices_cfg(ds, &B, &C);
    if (!((B == 64 || B == 128 || B == 256 || B == 512) && (C == 2 || C == 4 || C == 8))) return false;
    return 4 * sl_lds_bytes(ds->N, 2, B) <= 160 * 1024;            // (N = 1024, 512 threads: 4 x 39072 bytes)
}

// ms[0] -> slot[0], ms[1] -> slot[1] (different slots), both eligible and batch-compatible: one launch of k_slices_batch<B, C, 2,
// DEFER> on the current lane with launch_slices' (B, C); both slots are marked pending with that B.
nhp_status nhp_launch_slices_pair(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *const *ms, const int32_t *slot)
{
    // (k_slices_batch<., ., 2, DEFER> is compiled for items that are all their node's first: nhp_slices_pair_eligible's rule)
    if (!ds->all_sole) { nhp_set_error(ctx, "paired enqueue: the dataset has nodes with more than one item"); return NHP_EINVAL; }
    int B, C;
    slices_cfg(ds, &B, &C);
    const size_t lds = sl_lds_bytes(ds->N, 2, B);
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    for (int k = 0; k < 2; ++k) NHP_TRY(nhp_ctx_reserve_slot_partials(ctx, slot[k], 2 * (size_t)ds->n_items));
    nhp_cont_args a = nhp_make_args(ds, ms[0]);
    NHP_TRY(ensure_slices(ctx, ds, a));
    const nhp_slices sl = slices_view(ds);
    nhp_sets st;
    for (int k = 0; k < NHP_SETS_MAX; ++k) {
        const nhp_cont_model *m = ms[k & 1];
        st.p1[k] = m->d_p1; st.W[k] = m->d_W; st.A[k] = m->has_A ? m->d_A : nullptr; st.lambda0[k] = m->d_lambda0;
        st.out[k] = ctx->d_slot_partials[slot[k & 1]];
    }
    dim3 grid((unsigned)ds->n_items);
    bool ok = false;
#define NHP_PCASE(b, cc)                                                                                              \
    if (!ok && B == b && C == cc) {                                                                                   \
        ok = true;                                                                                                    \
        if (lds > 64 * 1024)                                                                                          \
            (void)hipFuncSetAttribute((const void *)k_slices_batch<b, cc, 2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        hipLaunchKernelGGL((k_slices_batch<b, cc, 2, true>), grid, dim3(b), lds, ctx->lane(), a, sl, st, (double *)nullptr,  \
                           (unsigned int *)nullptr);                                                                  \
    }
#define NHP_PROW(b) NHP_PCASE(b, 2) NHP_PCASE(b, 4) NHP_PCASE(b, 8)
    NHP_PROW(64) NHP_PROW(128) NHP_PROW(256) NHP_PROW(512)
#undef NHP_PROW
#undef NHP_PCASE
    if (!ok) { nhp_set_error(ctx, "paired enqueue: no kernel for %d threads, %d rows", B, C); return NHP_EINVAL; }
    NHP_HIP(ctx, hipGetLastError());
    for (int k = 0; k < 2; ++k) ctx->pend.mark(slot[k], ds->n_items, B);
    return NHP_OK;
}

// the planes of logit(x) and 1/(x(1-x)), made at the first call that wants them (data only); *ok = false: no room
static nhp_status ensure_lq_planes(nhp_ctx *ctx, nhp_cont_dataset *ds, const nhp_cont_args &a, const nhp_slices &sl, bool *ok)
{
    *ok = true;
    if (ds->d_sl_L) return NHP_OK;
    const size_t n = ((size_t)ds->sl_rows + 16) * 64;
    if (hipMalloc((void **)&ds->d_sl_L, 8 * n) != hipSuccess || hipMalloc((void **)&ds->d_sl_Q, 8 * n) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(ds->d_sl_L); (void)hipFree(ds->d_sl_Q);
        ds->d_sl_L = nullptr; ds->d_sl_Q = nullptr;
        *ok = false;
        return NHP_OK;
    }
    NHP_HIP(ctx, hipMemsetAsync(ds->d_sl_L + (size_t)ds->sl_rows * 64, 0, 8 * 16 * 64, ctx->main()));
    NHP_HIP(ctx, hipMemsetAsync(ds->d_sl_Q + (size_t)ds->sl_rows * 64, 0, 8 * 16 * 64, ctx->main()));
    hipLaunchKernelGGL(k_slices_build_lq, dim3((unsigned)ds->n_items), dim3(256), 0, ctx->main(), a, sl, ds->d_sl_L, ds->d_sl_Q);
    NHP_HIP(ctx, hipGetLastError());
    return NHP_OK;
}

nhp_status nhp_launch_sampler_slices(nhp_ctx *ctx, const nhp_cont_dataset *cds, const nhp_cont_model *m, const double *d_u, uint64_t seed,
                                     uint64_t step, int64_t *parents, int64_t *pnodes, int32_t *pn_b, double *dt_b, int *d_err, bool *launched)
{
    *launched = false;
    // (only windows below Julia's pairwise-sum threshold: the slice kernel sums sequentially)
    const bool expo = m->impulse_kind == NHP_IMPULSE_EXPONENTIAL;
    if (!cds->d_sl_row || cds->n_items <= 0 || (!expo && m->impulse_kind != NHP_IMPULSE_LOGITNORMAL) || cds->sl_max_rows + 1 > 1024) return NHP_OK;
    if (nhp_slices_off("NHP_SAMPLER_SLICES")) return NHP_OK;
    int B = 512, CACHE = 8;
    if (const char *cfg = getenv("NHP_SAMPLER_CFG")) sscanf(cfg, "%d,%d", &B, &CACHE);
    if (!((B == 256 || B == 512) && (CACHE == 8 || CACHE == 16))) { B = 512; CACHE = 8; }
    const size_t lds = 24 * ((size_t)cds->N + 1) + 8 * (size_t)(B / 64) * CACHE * 64;
    if (lds > 160 * 1024) return NHP_OK;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    nhp_cont_args a = nhp_make_args(cds, m);
    NHP_TRY(ensure_slices(ctx, cds, a));
    nhp_cont_dataset *ds = const_cast<nhp_cont_dataset *>(cds);
    const nhp_slices sl = slices_view(ds);
    if (expo && !ds->d_sl_D) {
        const size_t n = ((size_t)ds->sl_rows + 16) * 64;
        if (hipMalloc((void **)&ds->d_sl_D, 8 * n) != hipSuccess) { (void)hipGetLastError(); ds->d_sl_D = nullptr; return NHP_OK; }
        NHP_HIP(ctx, hipMemsetAsync(ds->d_sl_D + (size_t)ds->sl_rows * 64, 0, 8 * 16 * 64, ctx->main()));
        hipLaunchKernelGGL(k_slices_build_d, dim3((unsigned)ds->n_items), dim3(256), 0, ctx->main(), a, sl, ds->d_sl_D);
        NHP_HIP(ctx, hipGetLastError());
    }
    if (!expo) {
        bool planes = false;
        NHP_TRY(ensure_lq_planes(ctx, ds, a, sl, &planes));
        if (!planes) return NHP_OK;                                 // no room: the caller keeps its other kernel
    }
    dim3 grid((unsigned)ds->n_items);
#define NHP_SAMP(b, cc)                                                                                                \
    do {                                                                                                               \
        if (expo) {                                                                                                    \
            if (lds > 64 * 1024)                                                                                       \
                (void)hipFuncSetAttribute((const void *)k_sampler_slices<b, cc, NHP_IMPULSE_EXPONENTIAL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            hipLaunchKernelGGL((k_sampler_slices<b, cc, NHP_IMPULSE_EXPONENTIAL>), grid, dim3(b), lds, ctx->main(), a, sl, (const double *)ds->d_sl_D, \
                               (const double *)nullptr, d_u, seed, step, parents, pnodes, pn_b, dt_b, d_err);      \
        } else {                                                                                                       \
            if (lds > 64 * 1024)                                                                                       \
                (void)hipFuncSetAttribute((const void *)k_sampler_slices<b, cc, NHP_IMPULSE_LOGITNORMAL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            hipLaunchKernelGGL((k_sampler_slices<b, cc, NHP_IMPULSE_LOGITNORMAL>), grid, dim3(b), lds, ctx->main(), a, sl, (const double *)ds->d_sl_L, \
                               (const double *)ds->d_sl_Q, d_u, seed, step, parents, pnodes, pn_b, dt_b, d_err);      \
        }                                                                                                              \
    } while (0)
    if (B == 256 && CACHE == 8) NHP_SAMP(256, 8); else if (B == 256) NHP_SAMP(256, 16);
    else if (CACHE == 8) NHP_SAMP(512, 8); else NHP_SAMP(512, 16);
#undef NHP_SAMP
    NHP_HIP(ctx, hipGetLastError());
    *launched = true;
    return NHP_OK;
}
