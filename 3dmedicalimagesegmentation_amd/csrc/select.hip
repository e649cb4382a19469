// Exact order statistic of an fp32 array in device memory: a radix select over the bit pattern (include/unetr_hip.h:
// unetr_select_kth).
//
// Order: the unsigned key  bits ^ (sign ? 0xFFFFFFFF : 0x80000000)  -- a total order of every fp32 pattern: -inf < negatives < -0 <
// +0 < denormals < positives < +inf, NaNs at the two ends.  "r-th largest" is the r-th smallest of the complemented key.
//
// Four passes of 8 bits, most significant digit first.  A fixed sequence of six launches:
//   select_init_kernel        zeroes the four 256-bin histograms of the scratch and writes state[0] = (prefix 0, rank r)
//   select_hist_kernel<0..3>  one workgroup per 4096-element chunk, at most 1024 workgroups (above 4 Mi elements they stride over the
//                             chunks).  Pass p > 0 starts with the pick of pass p-1 -- EVERY workgroup scans the complete
//                             histogram p-1 (256 bins, one per thread) for the bin the remaining rank falls into, which gives the
//                             prefix and the rank inside that bin; workgroup 0 also writes them to state[p].  Then it counts digit
//                             p of the elements whose higher digits equal the prefix into an LDS histogram and adds its non-zero
//                             bins to histogram p with integer atomics.
//   select_final_kernel       the pick of pass 3 -> the key, n_equal = that bin's count, n_beyond = r - (rank inside the bin)
// No kernel waits for another workgroup: what a pass needs from its predecessor is complete when it starts.  Integer counts only, so
// the result is bitwise reproducible.  Every histogram word that is read was zeroed by select_init_kernel of the same call.
//
// LDS contention: the first digit of a loss map is sign + 7 exponent bits -- a handful of bins, so the lanes of a wave add to the
// same LDS word.  The first pass therefore keeps SEL_COPIES histogram copies per workgroup (lane l adds to copy l % SEL_COPIES) and
// a thread merges equal digits among the four elements of its 16-byte load into one add: 7.8 - 8.5 us against 9.8 - 10.0 us for one
// copy and one add per element, on the loss map of 2 x 14 x 96^3 (profiles/topk_loss.txt, section 4).  The later digits are
// mantissa bits, spread over the bins: there the copies only cost (their zeroing and summing: +0.6 to +1.3 us per pass, measured),
// so passes 1..3 run one copy.  UNETR_SELECT_PLAIN_HIST runs the first pass that way too, for that measurement.
//
// Loads: 16 bytes per thread when n % 4 == 0 and x is 16-byte aligned, else one element per thread; every access is below n.
#include <algorithm>
#include "common.hpp"
#include "../../include/unetr_hip.h"

namespace {

// (the order key sel_key, the bin and pass counts and the scratch size SEL_WS_BYTES: common.hpp, shared with topk_loss.hip)
constexpr int SEL_THREADS = 256;                    // = SEL_BINS: the pick runs one bin per thread
constexpr int SEL_CHUNK = 4096;                     // elements per chunk: one per workgroup up to SEL_MAX_GRID chunks (n = 4 Mi),
constexpr int SEL_MAX_GRID = 1024;                  // above that the workgroups stride over the chunks
constexpr int SEL_COPIES = 8;

__device__ __forceinline__ uint32_t sel_unkey(uint32_t key, uint32_t flip) {
    key ^= flip;
    return (key >> 31) ? key ^ 0x80000000u : ~key;
}

// The bin of hist[256] that holds sorted position `rank`: the smallest d with hist[0] + .. + hist[d] > rank.  All SEL_THREADS
// threads call it; sh has 8 words.  rank_in = the position inside that bin, count = hist[d].
__device__ __forceinline__ void sel_pick(const uint32_t* hist, uint32_t rank, uint32_t* sh, uint32_t& digit, uint32_t& rank_in,
                                         uint32_t& count) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t c = hist[threadIdx.x];
    uint32_t incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    if (lane == 63) sh[wave] = incl;
    if (threadIdx.x == 0) { sh[4] = 0; sh[5] = 0; sh[6] = 0; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < SEL_THREADS / 64 - 1; ++w)
        if (w < wave) incl += sh[w];
    if (incl > rank && incl - c <= rank) { sh[4] = threadIdx.x; sh[5] = rank - (incl - c); sh[6] = c; }
    __syncthreads();
    digit = sh[4]; rank_in = sh[5]; count = sh[6];
}

__global__ void __launch_bounds__(SEL_THREADS)
select_init_kernel(uint32_t* __restrict__ ws, const int* __restrict__ rank_dev, int rank_host, long n) {
    for (int i = threadIdx.x; i < SEL_HIST_WORDS; i += SEL_THREADS) ws[i] = 0u;
    if (threadIdx.x == 0) {
        long r = rank_dev ? (long)*rank_dev : (long)rank_host;
        r = r < 0 ? 0 : r >= n ? n - 1 : r;
        ws[SEL_HIST_WORDS] = 0u;
        ws[SEL_HIST_WORDS + 1] = (uint32_t)r;
    }
}

template <int PASS, int COPIES>
__global__ void __launch_bounds__(SEL_THREADS)
select_hist_kernel(const uint32_t* __restrict__ x, long n, uint32_t flip, uint32_t* __restrict__ ws) {
    __shared__ uint32_t lh[COPIES][SEL_BINS];
    __shared__ uint32_t sh[8];
    constexpr int SHIFT = 24 - 8 * PASS;
    constexpr uint32_t MASK = PASS == 0 ? 0u : 0xFFFFFFFFu << (PASS == 0 ? 0 : SHIFT + 8);
    uint32_t prefix = 0u;
    if constexpr (PASS > 0) {
        uint32_t* st = ws + SEL_HIST_WORDS;
        uint32_t digit, rank_in, count;
        sel_pick(ws + (PASS - 1) * SEL_BINS, st[2 * (PASS - 1) + 1], sh, digit, rank_in, count);
        prefix = st[2 * (PASS - 1)] | (digit << (SHIFT + 8));
        if (blockIdx.x == 0 && threadIdx.x == 0) { st[2 * PASS] = prefix; st[2 * PASS + 1] = rank_in; }
    }
#pragma unroll
    for (int c = 0; c < COPIES; ++c) lh[c][threadIdx.x] = 0u;
    __syncthreads();
    uint32_t* my = lh[COPIES > 1 ? (threadIdx.x & (COPIES - 1)) : 0];
    const bool vec = (n & 3) == 0 && (((uintptr_t)x) & 15) == 0;
    const long nchunk = (n + SEL_CHUNK - 1) / SEL_CHUNK;
    for (long ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {          // more than one chunk each only above SEL_MAX_GRID chunks
        const long c0 = ch * SEL_CHUNK, c1 = std::min<long>(n, c0 + SEL_CHUNK);
        if (vec) {
            // SEL_CHUNK and n are multiples of 4: a group that starts below c1 ends below it
            for (long i = c0 + 4 * threadIdx.x; i < c1; i += 4 * SEL_THREADS) {
                const u32x4 v = *(const u32x4*)(x + i);
                int d[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t k = sel_key(v[e], flip);
                    d[e] = (k & MASK) == prefix ? (int)((k >> SHIFT) & 255u) : -1;
                }
                if constexpr (COPIES > 1) {
                    uint32_t run = 1u;                       // equal neighbours among the four become one add
#pragma unroll
                    for (int e = 1; e < 4; ++e) {
                        if (d[e] == d[e - 1]) { ++run; continue; }
                        if (d[e - 1] >= 0) atomicAdd(&my[d[e - 1]], run);
                        run = 1u;
                    }
                    if (d[3] >= 0) atomicAdd(&my[d[3]], run);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (d[e] >= 0) atomicAdd(&my[d[e]], 1u);
                }
            }
        } else {
            for (long i = c0 + threadIdx.x; i < c1; i += SEL_THREADS) {
                const uint32_t k = sel_key(x[i], flip);
                if ((k & MASK) == prefix) atomicAdd(&my[(k >> SHIFT) & 255u], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t tot = 0u;
#pragma unroll
    for (int c = 0; c < COPIES; ++c) tot += lh[c][threadIdx.x];
    if (tot) atomicAdd(&ws[PASS * SEL_BINS + threadIdx.x], tot);
}

__global__ void __launch_bounds__(SEL_THREADS)
select_final_kernel(const uint32_t* __restrict__ ws, uint32_t flip, unetr_select_result* __restrict__ out) {
    __shared__ uint32_t sh[8];
    const uint32_t* st = ws + SEL_HIST_WORDS;
    uint32_t digit, rank_in, count;
    sel_pick(ws + (SEL_PASSES - 1) * SEL_BINS, st[2 * (SEL_PASSES - 1) + 1], sh, digit, rank_in, count);
    if (threadIdx.x == 0) {
        const uint32_t key = st[2 * (SEL_PASSES - 1)] | digit;
        out->value = __builtin_bit_cast(float, sel_unkey(key, flip));
        out->n_beyond = st[1] - rank_in;
        out->n_equal = count;
    }
}

template <int COPIES>
void launch_passes(const uint32_t* x, long n, uint32_t flip, uint32_t* ws, hipStream_t st) {
    const dim3 grid(std::min(cdiv(n, SEL_CHUNK), SEL_MAX_GRID)), block(SEL_THREADS);
    hipLaunchKernelGGL((select_hist_kernel<0, COPIES>), grid, block, 0, st, x, n, flip, ws);
    hipLaunchKernelGGL((select_hist_kernel<1, 1>), grid, block, 0, st, x, n, flip, ws);
    hipLaunchKernelGGL((select_hist_kernel<2, 1>), grid, block, 0, st, x, n, flip, ws);
    hipLaunchKernelGGL((select_hist_kernel<3, 1>), grid, block, 0, st, x, n, flip, ws);
}

}  // namespace

extern "C" size_t unetr_select_workspace_bytes(long n) { return n >= 1 && n < (1L << 31) ? SEL_WS_BYTES : 0; }

extern "C" int unetr_select_kth(const float* x, long n, const int* rank, int rank_host, int flags, unetr_select_result* out, void* ws,
                                size_t ws_bytes, void* stream) {
    if (!x || !out || n < 1 || (flags & ~(UNETR_SELECT_LARGEST | UNETR_SELECT_PLAIN_HIST))) return UNETR_ERR_ARG;
    if (n >= (1L << 31)) return UNETR_ERR_UNSUPPORTED;
    if (!rank && (rank_host < 0 || rank_host >= n)) return UNETR_ERR_ARG;
    if (!ws || ((uintptr_t)ws & 15) || ws_bytes < SEL_WS_BYTES) return UNETR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    uint32_t* w = (uint32_t*)ws;
    const uint32_t flip = (flags & UNETR_SELECT_LARGEST) ? 0xFFFFFFFFu : 0u;
    hipLaunchKernelGGL(select_init_kernel, dim3(1), dim3(SEL_THREADS), 0, st, w, rank, rank_host, n);
    if (flags & UNETR_SELECT_PLAIN_HIST) launch_passes<1>((const uint32_t*)x, n, flip, w, st);
    else launch_passes<SEL_COPIES>((const uint32_t*)x, n, flip, w, st);
    hipLaunchKernelGGL(select_final_kernel, dim3(1), dim3(SEL_THREADS), 0, st, w, flip, out);
    return unetr_check_launch();
}
