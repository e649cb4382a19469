// Top-k cross entropy: the mean of the K largest per-voxel cross entropies of the whole batch (nnU-Net's TopKLoss), K = k % of the
// voxels that have a value.  (configuration: unetr_topkce_desc, include/unetr_hip.h)
//
//   u_v = w[y_v] * (logf(sum_c e^(z_c - max)) - (z_y - max))       the expression seg_loss.hip's seg_fwd_voxel uses
//   N = #voxels with a value over all B*V (an ignored voxel has none),  K = max(1, floor((double)N * (double)k / 100.0))
//   t = K-th largest u,  n_gt = #{u > t},  n_eq = #{u == t}
//   X = (sum_{u > t} u + (K - n_gt) * t) / K                         = torch.topk(u, K).values.mean()
//   dX/du_v = 1/K where u > t,  (K - n_gt) / (n_eq * K) where u == t,  0 elsewhere: ties at the threshold share the rest equally
//
// Forward, ten launches: topk_val_kernel (u into `values`, an ignored voxel as the sentinel -1; per-block counts of valued voxels),
// topk_rank_kernel (N, K, rank K-1 in device memory), the six launches of unetr_select_kth (largest, rank from device memory),
// topk_sum_kernel (fixed-order partial sums of the u above t) and topk_final_kernel (one block, in double).  Real values are >= 0,
// so a largest-K select with K <= N never reaches a sentinel, and the sum pass never takes one.  Backward, one launch, one voxel per
// thread: it compares the bits forward stored in `values` with t -- never a recomputed value -- and reads the logits only where the
// voxel's weight is not zero.  No float atomics: reproducible run to run.  Every access is bounded by V (or B*V).
// Channel dispatch, base pointers, alignment rule, target decode, softmax exponentials and block tails: voxel_loss.hpp; the order key
// and the size of the select's scratch: common.hpp.
#include <algorithm>
#include "voxel_loss.hpp"

namespace {

constexpr int TK_VPB = 1024;     // voxels per block of the value pass: four per thread
constexpr int TK_SPB = 4096;     // values per block of the sum pass (one partial each)
constexpr int TK_BVPB = 256;     // voxels per backward block: one per thread
constexpr float TK_SENTINEL = -1.f;
constexpr int TK_META_WORDS = 8; // rank, N, K, pad, then the unetr_select_result (3 words), pad

struct TkCfg {
    const float* cw;
    int has_ignore, ignore;
};

// a value's place in the order the select ran in (sel_key without the flip: larger value, larger key)
__device__ __forceinline__ uint32_t tk_key(float f) { return sel_key(__builtin_bit_cast(uint32_t, f), 0u); }

template <int C>
__device__ __forceinline__ float tk_voxel_value(const float (&z)[C], int lab, const TkCfg& cfg, const float (&w)[C]) {
    float e[C], mx;
    const float se = softmax_exp<C>(z, e, mx);
    float zl = 0.f, wl = 1.f;
#pragma unroll
    for (int c = 0; c < C; ++c)
        if (c == lab) zl = z[c];
    if (cfg.cw) {
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (c == lab) wl = w[c];
    }
    return wl * (logf(se) - (zl - mx));
}

template <int C, bool SIG>
__global__ void __launch_bounds__(256)
topk_val_kernel(const float* __restrict__ logits, const float* __restrict__ label, long V, TkCfg cfg, float* __restrict__ values,
                uint32_t* __restrict__ part_cnt) {
    __shared__ uint32_t red[4];
    const int b = blockIdx.y;
    const long v0 = (long)blockIdx.x * TK_VPB, v1 = std::min<long>(V, v0 + TK_VPB);
    const float* lg = item_channels<C>(logits, b, V);
    const float* lb = item_target<C, SIG>(label, b, V);
    float* val = values + (long)b * V;
    float w[C];
#pragma unroll
    for (int c = 0; c < C; ++c) w[c] = cfg.cw ? cfg.cw[c] : 1.f;
    uint32_t cnt = 0u;
    if (vec4_ok(V, logits, label, values)) {
        // TK_VPB and V are multiples of 4: a group that starts below v1 ends below it
        const long v = v0 + 4 * threadIdx.x;
        if (v < v1) {
            f32x4 zv[C], tv[SIG ? C : 1], uv;
#pragma unroll
            for (int c = 0; c < C; ++c) zv[c] = *(const f32x4*)(lg + (long)c * V + v);
            if constexpr (SIG) {
#pragma unroll
                for (int c = 0; c < C; ++c) tv[c] = *(const f32x4*)(lb + (long)c * V + v);
            } else {
                tv[0] = *(const f32x4*)(lb + v);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float z[C];
                int lab;
#pragma unroll
                for (int c = 0; c < C; ++c) z[c] = zv[c][e];
                bool valid = true;
                if constexpr (SIG) {
                    float t[C];
#pragma unroll
                    for (int c = 0; c < C; ++c) t[c] = tv[c][e];
                    lab = mask_argmax<C>(t);
                } else {
                    lab = (int)tv[0][e];
                    valid = !(cfg.has_ignore && lab == cfg.ignore);
                }
                uv[e] = valid ? tk_voxel_value<C>(z, lab, cfg, w) : TK_SENTINEL;
                cnt += valid ? 1u : 0u;
            }
            *(f32x4*)(val + v) = uv;
        }
    } else {
        for (long v = v0 + threadIdx.x; v < v1; v += 256) {
            float z[C];
            int lab;
            bool valid = true;
            if constexpr (SIG) {
                float t[C];
#pragma unroll
                for (int c = 0; c < C; ++c) t[c] = lb[(long)c * V + v];
                lab = mask_argmax<C>(t);
            } else {
                lab = (int)lb[v];
                valid = !(cfg.has_ignore && lab == cfg.ignore);
            }
#pragma unroll
            for (int c = 0; c < C; ++c) z[c] = lg[(long)c * V + v];
            val[v] = valid ? tk_voxel_value<C>(z, lab, cfg, w) : TK_SENTINEL;
            cnt += valid ? 1u : 0u;
        }
    }
    block_wave_sums<1>(&cnt, red);
    if (threadIdx.x == 0) part_cnt[(long)b * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// Single block: N from the per-block counts, K from N and *k, the select's rank K-1.  meta = {rank, N, K}
__global__ void __launch_bounds__(256)
topk_rank_kernel(const uint32_t* __restrict__ part_cnt, int nblk, const float* __restrict__ k, int* __restrict__ meta) {
    __shared__ uint32_t red[4];
    uint32_t cnt = 0u;
    for (int i = threadIdx.x; i < nblk; i += 256) cnt += part_cnt[i];
    block_wave_sums<1>(&cnt, red);
    if (threadIdx.x == 0) {
        const long N = (long)red[0] + red[1] + red[2] + red[3];
        long K = (long)floor((double)N * (double)*k / 100.0);
        K = std::max<long>(1, std::min<long>(K, N));
        meta[0] = (int)(K - 1); meta[1] = (int)N; meta[2] = (int)K; meta[3] = 0;
    }
}

__global__ void __launch_bounds__(256)
topk_sum_kernel(const float* __restrict__ values, long n, const unetr_select_result* __restrict__ sel, float* __restrict__ part_sum) {
    __shared__ float red[4];
    const uint32_t kt = tk_key(sel->value);
    const long i0 = (long)blockIdx.x * TK_SPB, i1 = std::min<long>(n, i0 + TK_SPB);
    float s = 0.f;
    if (vec4_ok(n, values)) {
        for (long i = i0 + 4 * threadIdx.x; i < i1; i += 1024) {
            const f32x4 u = *(const f32x4*)(values + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) s += tk_key(u[e]) > kt ? u[e] : 0.f;
        }
    } else {
        for (long i = i0 + threadIdx.x; i < i1; i += 256) {
            const float u = values[i];
            s += tk_key(u) > kt ? u : 0.f;
        }
    }
    block_wave_sums<1>(&s, red);
    if (threadIdx.x == 0) part_sum[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// Single block.  out = {X, t, K, N}; coef = {1/K, (K - n_gt) / (n_eq K), t, 0}
__global__ void __launch_bounds__(256)
topk_final_kernel(const float* __restrict__ part_sum, int nsum, const int* __restrict__ meta, const unetr_select_result* __restrict__ sel,
                  float* __restrict__ out, float* __restrict__ coef) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nsum; i += 256) s += (double)part_sum[i];
    block_wave_sums<1>(&s, red);
    if (threadIdx.x == 0) {
        s = red[0] + red[1] + red[2] + red[3];
        const double K = (double)meta[2], t = (double)sel->value;
        const double rest = K - (double)sel->n_beyond, n_eq = (double)sel->n_equal;
        out[0] = (float)((s + rest * t) / K); out[1] = sel->value; out[2] = (float)K; out[3] = (float)meta[1];
        coef[0] = (float)(1.0 / K); coef[1] = (float)(rest / (n_eq * K)); coef[2] = sel->value; coef[3] = 0.f;
    }
}

template <int C, bool SIG>
__global__ void __launch_bounds__(256)
topk_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ label, const float* __restrict__ values,
                const float* __restrict__ coef, const float* __restrict__ dloss, float* __restrict__ dlogits, long V, TkCfg cfg) {
    const int b = blockIdx.y;
    const long v = (long)blockIdx.x * TK_BVPB + threadIdx.x;
    if (v >= V) return;
    float* dl = item_channels<C>(dlogits, b, V);
    const uint32_t ku = tk_key(values[(long)b * V + v]), kt = tk_key(coef[2]);
    float g = ku > kt ? coef[0] : ku == kt ? coef[1] : 0.f;
    if (g == 0.f) {                                  // below the threshold, or ignored (the sentinel is below every real value)
#pragma unroll
        for (int c = 0; c < C; ++c) dl[(long)c * V + v] = 0.f;
        return;
    }
    const float* lg = item_channels<C>(logits, b, V);
    const float* lb = item_target<C, SIG>(label, b, V);
    int lab;
    if constexpr (SIG) {
        float t[C];
#pragma unroll
        for (int c = 0; c < C; ++c) t[c] = lb[(long)c * V + v];
        lab = mask_argmax<C>(t);
    } else {
        lab = (int)lb[v];
    }
    float z[C], e[C], mx;
#pragma unroll
    for (int c = 0; c < C; ++c) z[c] = lg[(long)c * V + v];
    const float se = softmax_exp<C>(z, e, mx);
    float wl = 1.f;
    if (cfg.cw) {
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (c == lab) wl = cfg.cw[c];
    }
    g *= (dloss ? *dloss : 1.f) * wl;
    const float inv = 1.f / se;
#pragma unroll
    for (int c = 0; c < C; ++c) dl[(long)c * V + v] = g * (e[c] * inv - (c == lab ? 1.f : 0.f));
}

int check_desc(const unetr_topkce_desc* d) {
    if (int rc = check_voxel_desc(d)) return rc;
    if ((long)d->B * d->V >= (1L << 31)) return UNETR_ERR_UNSUPPORTED;
    if (d->multilabel && (d->has_ignore || d->class_weight)) return UNETR_ERR_UNSUPPORTED;
    return UNETR_OK;
}

TkCfg make_cfg(const unetr_topkce_desc* d) {
    TkCfg cfg;
    cfg.cw = d->class_weight;
    cfg.has_ignore = !d->multilabel && d->has_ignore;
    cfg.ignore = d->ignore_index;
    return cfg;
}

}  // namespace

extern "C" size_t unetr_topkce_workspace_bytes(const unetr_topkce_desc* d) {
    if (check_desc(d) != UNETR_OK) return 0;
    const size_t n = SEL_WS_BYTES + TK_META_WORDS * 4 + 4 * (size_t)d->B * cdiv(d->V, TK_VPB) + 4 * (size_t)cdiv((long)d->B * d->V, TK_SPB);
    return (n + 15) & ~(size_t)15;
}

extern "C" int unetr_topkce_fwd(const unetr_topkce_desc* d, const float* logits, const float* label, const float* k, float* values,
                                float* out, float* coef, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_desc(d)) return rc;
    if (!logits || !label || !k || !values || !out || !coef) return UNETR_ERR_ARG;
    if (!ws || ((uintptr_t)ws & 15) || unetr_topkce_workspace_bytes(d) > ws_bytes) return UNETR_ERR_WORKSPACE;
    const int B = d->B, nchunk = cdiv(d->V, TK_VPB), nblk = B * nchunk;
    const long V = d->V, n = (long)B * V;
    const int nsum = cdiv(n, TK_SPB);
    const TkCfg cfg = make_cfg(d);
    int* meta = (int*)((char*)ws + SEL_WS_BYTES);
    unetr_select_result* sel = (unetr_select_result*)(meta + 4);
    uint32_t* part_cnt = (uint32_t*)(meta + TK_META_WORDS);
    float* part_sum = (float*)(part_cnt + nblk);
    hipStream_t st = (hipStream_t)stream;
    VOXEL_DISPATCH(d->C, d->multilabel, hipLaunchKernelGGL((topk_val_kernel<CC, SIG>), dim3(nchunk, B), dim3(256), 0, st, logits, label, V, cfg,
                                                           values, part_cnt));
    hipLaunchKernelGGL(topk_rank_kernel, dim3(1), dim3(256), 0, st, part_cnt, nblk, k, meta);
    if (int rc = unetr_select_kth(values, n, meta, 0, UNETR_SELECT_LARGEST, sel, ws, SEL_WS_BYTES, stream)) return rc;
    hipLaunchKernelGGL(topk_sum_kernel, dim3(nsum), dim3(256), 0, st, values, n, sel, part_sum);
    hipLaunchKernelGGL(topk_final_kernel, dim3(1), dim3(256), 0, st, part_sum, nsum, meta, sel, out, coef);
    return unetr_check_launch();
}

extern "C" int unetr_topkce_bwd(const unetr_topkce_desc* d, const float* logits, const float* label, const float* values,
                                const float* coef, const float* dloss, float* dlogits, void* stream) {
    if (int rc = check_desc(d)) return rc;
    if (!logits || !label || !values || !coef || !dlogits) return UNETR_ERR_ARG;
    const int B = d->B, nblk = cdiv(d->V, TK_BVPB);
    const long V = d->V;
    const TkCfg cfg = make_cfg(d);
    hipStream_t st = (hipStream_t)stream;
    VOXEL_DISPATCH(d->C, d->multilabel, hipLaunchKernelGGL((topk_bwd_kernel<CC, SIG>), dim3(nblk, B), dim3(256), 0, st, logits, label, values,
                                                           coef, dloss, dlogits, V, cfg));
    return unetr_check_launch();
}
