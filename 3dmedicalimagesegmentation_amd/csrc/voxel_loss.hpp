// What the per-voxel segmentation losses share (loss.hip, seg_loss.hip, dist_loss.hip, topk_loss.hip): logits [B][C][V] against a
// target that is either class ids [B][V] or, with SIG, a float mask [B][C][V]; C is a template parameter up to VOXEL_MAXC; blocks
// of 256 threads with the batch item in blockIdx.y.  Everything here is either glue without arithmetic or one fixed piece of
// arithmetic (softmax_exp, mask_argmax).  What a loss does with the exponentials, and each forward kernel's walk over its voxels,
// stay in its own file: the accumulations there are `acc += a * b` under the compiler's default contraction, and which of them
// become one fma and which a multiply and an add -- a rounding -- follows the shape of the code around them.
#pragma once
#include "common.hpp"

constexpr int VOXEL_MAXC = 16;

// ---- host: the opening of every entry point's argument check, and the run-time (C, multilabel) -> compile-time dispatch
static inline int check_voxel_dims(int B, int C, long V, bool b_on_grid_y = true) {
    if (B <= 0 || V <= 0 || (b_on_grid_y && B > 65535)) return UNETR_ERR_ARG;
    if (C < 1 || C > VOXEL_MAXC) return UNETR_ERR_UNSUPPORTED;
    return UNETR_OK;
}
template <class D>
static inline int check_voxel_desc(const D* d) { return d ? check_voxel_dims(d->B, d->C, d->V) : UNETR_ERR_ARG; }

// run the statement with `CC` bound to the channel count and `SIG` to the target form; C beyond VOXEL_MAXC: return UNETR_ERR_UNSUPPORTED
#define VOXEL_CASE_(N, ...) case N: { constexpr int CC = N; __VA_ARGS__; } break;
#define VOXEL_SWITCH_(C_, ...)                                                                                                      \
    switch (C_) {                                                                                                                   \
        VOXEL_CASE_(1, __VA_ARGS__) VOXEL_CASE_(2, __VA_ARGS__) VOXEL_CASE_(3, __VA_ARGS__) VOXEL_CASE_(4, __VA_ARGS__)             \
        VOXEL_CASE_(5, __VA_ARGS__) VOXEL_CASE_(6, __VA_ARGS__) VOXEL_CASE_(7, __VA_ARGS__) VOXEL_CASE_(8, __VA_ARGS__)             \
        VOXEL_CASE_(9, __VA_ARGS__) VOXEL_CASE_(10, __VA_ARGS__) VOXEL_CASE_(11, __VA_ARGS__) VOXEL_CASE_(12, __VA_ARGS__)          \
        VOXEL_CASE_(13, __VA_ARGS__) VOXEL_CASE_(14, __VA_ARGS__) VOXEL_CASE_(15, __VA_ARGS__) VOXEL_CASE_(16, __VA_ARGS__)         \
        default: return UNETR_ERR_UNSUPPORTED;                                                                                      \
    }
#define VOXEL_DISPATCH(C_, multilabel, ...)                                             \
    do {                                                                                \
        if (multilabel) { constexpr bool SIG = true; VOXEL_SWITCH_(C_, __VA_ARGS__) }   \
        else { constexpr bool SIG = false; VOXEL_SWITCH_(C_, __VA_ARGS__) }             \
    } while (0)

// ---- one batch item's part of a tensor: [C][V] (logits, mask, dlogits, a per-channel side tensor), or the target in its form
template <int C, class T>
__device__ __forceinline__ T* item_channels(T* p, int b, long V) { return p + (long)b * C * V; }
template <int C, bool SIG>
__device__ __forceinline__ const float* item_target(const float* t, int b, long V) { return t + (SIG ? (long)b * C * V : (long)b * V); }

// 16-byte accesses at every multiple of four voxels: V is a multiple of 4 and each of the tensors starts 16-byte aligned
template <class... T>
__host__ __device__ __forceinline__ bool vec4_ok(long V, const T*... p) { return (V & 3) == 0 && ((... | (uintptr_t)p) & 15) == 0; }

// ---- target of one voxel as t[C] (one-hot of the label, or the mask) and its class (the label, or the first maximal channel of
// the mask: torch.argmax's rule)
template <int C>
__device__ __forceinline__ void onehot_target(int lab, float (&t)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) t[c] = c == lab ? 1.f : 0.f;
}
template <int C>
__device__ __forceinline__ int mask_argmax(const float (&t)[C]) {
    float tmax = -3.0e38f;
    int lab = 0;
#pragma unroll
    for (int c = 0; c < C; ++c)
        if (t[c] > tmax) { tmax = t[c]; lab = c; }
    return lab;
}

// mx = max_c z[c], e[c] = expf(z[c] - mx), returns their sum in channel order (e may be z itself: the maximum is complete first)
template <int C>
__device__ __forceinline__ float softmax_exp(const float (&z)[C], float (&e)[C], float& mx) {
    mx = -3.0e38f;
#pragma unroll
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, z[c]);
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { e[c] = expf(z[c] - mx); se += e[c]; }
    return se;
}

// ---- block tail: every wave's sum of each of the N accumulators into red[wave][0..N), then the barrier.  What combines the waves
// (and in which order) stays with the caller.
__device__ __forceinline__ float wave_add(float v) { return wave_sum(v); }
__device__ __forceinline__ double wave_add(double v) { return wave_sum_d(v); }
__device__ __forceinline__ uint32_t wave_add(uint32_t v) { return wave_sum_u(v); }
template <int N, class T>
__device__ __forceinline__ void block_wave_sums(const T* acc, T* red /* [waves][N] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const T s = wave_add(acc[i]);
        if (lane == 0) red[wave * N + i] = s;
    }
    __syncthreads();
}
