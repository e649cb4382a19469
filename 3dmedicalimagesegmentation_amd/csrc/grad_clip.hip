// Gradient clipping by global L2 norm on the device (include/unetr_hip.h: unetr_grad_sumsq_ranges and the entry points after it;
// torch.nn.utils.clip_grad_norm_ semantics, error_if_nonfinite=False).
//
//   grad_sumsq_kernel<B16>   one workgroup per 8192-element block of a range [lo, hi) of a flat gradient source (fp32, or bf16: the
//                            data-parallel communication buffer).  Every element is widened to double, squared and accumulated in
//                            double: the product of two fp32 numbers is exact in double and the sum of <= 1e8 positive terms loses
//                            ~1e-8 relative, so the fp32 norm is within 1 ulp of the correctly rounded one whatever the data.  The
//                            workgroup's sum goes to the workspace slot of its block index.  No atomics: the order of every
//                            addition is a function of the shapes alone, the result is bitwise reproducible.
//   grad_clip_finalize_kernel one workgroup adds the slots in a fixed order and writes the clip row {norm, coef, max_norm, nonfinite}:
//                            norm = float(gscale * sqrt(S)), coef = min(1, max_norm / (norm + 1e-6)) in fp32 as torch computes it
//                            (NaN stays NaN), max_norm READ from the row -- a captured step follows unetr_grad_clip_set.
//   grad_scale_kernel        g *= coef over the same ranges (the free function clip_grad_norm_; the optimizer instead hands the
//                            coefficient to unetr_adamw_hyper_clip and never rewrites the gradients).
//
// Ranges: a device table of (lo, hi, first_block) rows like unetr_cast_bf16_ranges, or one range by value (the per-tensor forms).
// Loads are 16 bytes per lane over the whole vectors INSIDE [lo, hi) -- the base pointer is 16-byte aligned, a range that does not
// start or end on a vector boundary gets a scalar head / tail -- so nothing outside a range is ever read: the gaps of the arena hold
// stale gradients of parameters that are not part of the step.
#include <algorithm>
#include <cmath>
#include "common.hpp"
#include "../../include/unetr_hip.h"

namespace {

constexpr int GC_THREADS = 256;
constexpr long GC_BLOCK = 8192;                      // elements per workgroup = per partial slot (8 f32x4 / 4 bf16x8 loads per thread)

__device__ __forceinline__ double sq(float x) { const double d = (double)x; return d * d; }
__device__ __forceinline__ float bf16_bits_to_float(uint32_t hi16) { return __builtin_bit_cast(float, hi16 << 16); }

template <bool B16> struct Src;
template <> struct Src<false> {
    static constexpr int V = 4;
    static __device__ __forceinline__ double one(const void* s, long i) { return sq(((const float*)s)[i]); }
    static __device__ __forceinline__ double vec(const void* s, long v) {
        const f32x4 a = ((const f32x4*)s)[v];
        return ((sq(a[0]) + sq(a[1])) + sq(a[2])) + sq(a[3]);
    }
};
template <> struct Src<true> {
    static constexpr int V = 8;
    static __device__ __forceinline__ double one(const void* s, long i) { return sq(bf16_bits_to_float(((const uint16_t*)s)[i])); }
    static __device__ __forceinline__ double vec(const void* s, long v) {
        const u32x4 a = ((const u32x4*)s)[v];
        double r = 0.0;
#pragma unroll
        for (int e = 0; e < 4; ++e) r = (r + sq(bf16_bits_to_float(a[e] & 0xffffu))) + sq(__builtin_bit_cast(float, a[e] & 0xffff0000u));
        return r;
    }
};

// the range row of workgroup `blk`: last row whose first block <= blk (uniform: scalar loads)
__device__ __forceinline__ void range_of(const long* __restrict__ table, int nr, long blk, long lo1, long hi1, long& beg, long& end) {
    long lo = lo1, hi = hi1, first = 0;
    if (table) {
        int lo_r = 0, hi_r = nr - 1;
        while (lo_r < hi_r) {
            const int mid = (lo_r + hi_r + 1) >> 1;
            if (table[3 * mid + 2] <= blk) lo_r = mid; else hi_r = mid - 1;
        }
        lo = table[3 * lo_r]; hi = table[3 * lo_r + 1]; first = table[3 * lo_r + 2];
    }
    beg = lo + (blk - first) * GC_BLOCK;
    end = min(hi, beg + GC_BLOCK);
    if (end < beg) end = beg;                         // (a block past its range's end: nothing to do, the slot gets 0)
}

// sum over the workgroup in a fixed order: xor tree inside each wave, then the four wave sums in order
__device__ __forceinline__ double block_sum(double s, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = s;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

template <bool B16>
__global__ void __launch_bounds__(GC_THREADS)
grad_sumsq_kernel(const void* __restrict__ src, const long* __restrict__ table, int nr, long lo1, long hi1, double* __restrict__ partials) {
    constexpr int V = Src<B16>::V;
    __shared__ double sh[GC_THREADS / 64];
    long beg, end;
    range_of(table, nr, blockIdx.x, lo1, hi1, beg, end);
    const long vbeg = (beg + V - 1) / V, vend = end / V;          // whole vectors inside [beg, end)
    double s = 0.0;
    if (vbeg >= vend) {                                            // shorter than one aligned vector
        for (long i = beg + threadIdx.x; i < end; i += GC_THREADS) s += Src<B16>::one(src, i);
    } else {
        if (vend - vbeg == GC_BLOCK / V) {                         // a full aligned block: every load is issued before the first add
            constexpr int PER = GC_BLOCK / V / GC_THREADS;
            double t[PER];
#pragma unroll
            for (int k = 0; k < PER; ++k) t[k] = Src<B16>::vec(src, vbeg + threadIdx.x + (long)k * GC_THREADS);
#pragma unroll
            for (int k = 0; k < PER; ++k) s += t[k];
        } else {
            for (long v = vbeg + threadIdx.x; v < vend; v += GC_THREADS) s += Src<B16>::vec(src, v);
        }
        const long head = vbeg * V - beg, tail = end - vend * V;   // < V each
        if ((long)threadIdx.x < head) s += Src<B16>::one(src, beg + threadIdx.x);
        if ((long)threadIdx.x < tail) s += Src<B16>::one(src, vend * V + threadIdx.x);
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ void __launch_bounds__(GC_THREADS)
grad_clip_finalize_kernel(const double* __restrict__ partials, long n, float gscale, float* __restrict__ row) {
#pragma clang fp contract(off)
    __shared__ double sh[GC_THREADS / 64];
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += GC_THREADS) s += partials[i];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) {
        const float norm = (float)((double)gscale * sqrt(s));
        const float c = row[2] / (norm + 1e-6f);
        row[0] = norm;
        row[1] = c >= 1.0f ? 1.0f : c;                              // = c < 1 ? c : 1 for every number, and NaN stays NaN (no fminf)
        if (!(fabsf(norm) < INFINITY)) row[3] += 1.0f;
    }
}

__global__ void grad_clip_set_kernel(float* __restrict__ row, float max_norm) {
    if (threadIdx.x == 0 && blockIdx.x == 0) row[2] = max_norm;
}

__global__ void __launch_bounds__(GC_THREADS)
grad_scale_kernel(float* __restrict__ g, const long* __restrict__ table, int nr, long lo1, long hi1, long n_blocks, const float* __restrict__ coef_dev) {
#pragma clang fp contract(off)
    const float coef = *coef_dev;                                   // wave-uniform: one scalar load
    if (coef == 1.0f) return;                                       // x * 1 = x for every x: nothing to rewrite
    for (long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        long beg, end;
        range_of(table, nr, blk, lo1, hi1, beg, end);
        const long vbeg = (beg + 3) / 4, vend = end / 4;
        if (vbeg >= vend) {
            for (long i = beg + threadIdx.x; i < end; i += GC_THREADS) g[i] = g[i] * coef;
            continue;
        }
        for (long v = vbeg + threadIdx.x; v < vend; v += GC_THREADS) ((f32x4*)g)[v] = ((const f32x4*)g)[v] * coef;
        const long head = vbeg * 4 - beg, tail = end - vend * 4;
        if ((long)threadIdx.x < head) g[beg + threadIdx.x] = g[beg + threadIdx.x] * coef;
        if ((long)threadIdx.x < tail) g[vend * 4 + threadIdx.x] = g[vend * 4 + threadIdx.x] * coef;
    }
}

int sumsq_launch(const void* src, int b16, const long* table, int nr, long lo, long hi, long n_blocks, double* partials, size_t partials_bytes,
                 void* stream) {
    if (!src || !partials || n_blocks <= 0 || ((uintptr_t)src & 15) || ((uintptr_t)partials & 7)) return UNETR_ERR_ARG;
    if (n_blocks > 0x7fffffffL) return UNETR_ERR_UNSUPPORTED;
    if ((size_t)n_blocks * sizeof(double) > partials_bytes) return UNETR_ERR_WORKSPACE;
    if (b16)
        hipLaunchKernelGGL(grad_sumsq_kernel<true>, dim3((unsigned)n_blocks), dim3(GC_THREADS), 0, (hipStream_t)stream, src, table, nr, lo, hi, partials);
    else
        hipLaunchKernelGGL(grad_sumsq_kernel<false>, dim3((unsigned)n_blocks), dim3(GC_THREADS), 0, (hipStream_t)stream, src, table, nr, lo, hi, partials);
    return unetr_check_launch();
}

int scale_launch(float* g, const long* table, int nr, long lo, long hi, long n_blocks, const float* coef_dev, void* stream) {
    if (!g || !coef_dev || n_blocks <= 0 || ((uintptr_t)g & 15) || ((uintptr_t)coef_dev & 3)) return UNETR_ERR_ARG;
    const unsigned grid = (unsigned)std::min<long>(n_blocks, 4096);
    hipLaunchKernelGGL(grad_scale_kernel, dim3(grid), dim3(GC_THREADS), 0, (hipStream_t)stream, g, table, nr, lo, hi, n_blocks, coef_dev);
    return unetr_check_launch();
}

}  // namespace

extern "C" int unetr_grad_sumsq_ranges(const void* src_arena, int src_is_bf16, const long* table_dev, int n_ranges, long n_blocks,
                                       double* partials, size_t partials_bytes, void* stream) {
    if (!table_dev || n_ranges <= 0) return UNETR_ERR_ARG;
    return sumsq_launch(src_arena, src_is_bf16, table_dev, n_ranges, 0, 0, n_blocks, partials, partials_bytes, stream);
}

// one tensor of n elements at any element-aligned address: the base is aligned down to 16 bytes and the range starts that many
// elements in, so the vector loads stay aligned and inside the tensor
extern "C" int unetr_grad_sumsq(const void* src, int src_is_bf16, long n, double* partials, size_t partials_bytes, void* stream) {
    const int esz = src_is_bf16 ? 2 : 4;
    if (!src || n <= 0 || ((uintptr_t)src & (esz - 1))) return UNETR_ERR_ARG;
    const long shift = (long)(((uintptr_t)src & 15) / esz);
    return sumsq_launch((const char*)src - shift * esz, src_is_bf16, nullptr, 0, shift, shift + n, (n + GC_BLOCK - 1) / GC_BLOCK, partials,
                        partials_bytes, stream);
}

extern "C" int unetr_grad_clip_finalize(const double* partials, long n_partials, float gscale, float* clip_row, void* stream) {
    if (!partials || !clip_row || n_partials <= 0 || ((uintptr_t)partials & 7) || ((uintptr_t)clip_row & 3)) return UNETR_ERR_ARG;
    hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(GC_THREADS), 0, (hipStream_t)stream, partials, n_partials, gscale, clip_row);
    return unetr_check_launch();
}

extern "C" int unetr_grad_clip_set(float* clip_row, float max_norm, void* stream) {
    if (!clip_row || ((uintptr_t)clip_row & 3) || !(max_norm > 0.f)) return UNETR_ERR_ARG;
    hipLaunchKernelGGL(grad_clip_set_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, clip_row, max_norm);
    return unetr_check_launch();
}

extern "C" int unetr_grad_scale_ranges(float* grad_arena, const long* table_dev, int n_ranges, long n_blocks, const float* coef_dev, void* stream) {
    if (!table_dev || n_ranges <= 0) return UNETR_ERR_ARG;
    return scale_launch(grad_arena, table_dev, n_ranges, 0, 0, n_blocks, coef_dev, stream);
}

extern "C" int unetr_grad_scale(float* g, long n, const float* coef_dev, void* stream) {
    if (!g || n <= 0 || ((uintptr_t)g & 3)) return UNETR_ERR_ARG;
    const long shift = (long)(((uintptr_t)g & 15) / 4);
    return scale_launch(g - shift, nullptr, 0, shift, shift + n, (n + GC_BLOCK - 1) / GC_BLOCK, coef_dev, stream);
}
