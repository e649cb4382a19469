// The distance-map losses on the fields of edt.hip (configuration: unetr_distloss_desc, include/unetr_hip.h):
//
//   BOUNDARY   (Kervadec et al. 2019)          L = w * mean over (b, included c, v) of  p * phi
//   HAUSDORFF  (Karimi & Salcudean 2019)       L = w * mean over (b, included c, v) of  (p - g)^2 * F
//
// p = softmax(logits, 1) with class-id targets, or sigmoid(logits) with a multilabel mask, as seg_loss.hip has them; phi is the
// signed field of the target, F = F_P^alpha + F_G^alpha the sum edt.hip accumulated (a constant of the gradient).  Both reduce to
// one coefficient per voxel and channel, a_c = phi_c or 2 (p_c - g_c) F_c (0 for an excluded channel, which still takes part in
// the softmax):
//   softmax   dz_k = w/N * p_k (a_k - sum_c p_c a_c)        sigmoid   dz_k = w/N * a_k p_k (1 - p_k)
// w is read from device memory by both kernels, so a captured step can be re-weighted between replays.
//
// Forward: one streaming pass (16-byte loads when V % 4 == 0 and every pointer is 16-byte aligned, one voxel per thread and
// iteration otherwise), one float partial per block from a fixed shuffle / LDS tree, then one block that adds the partials in
// double in a fixed order: reproducible run to run, no float atomics.  Backward: one pass, one voxel per thread, as
// segloss_bwd_kernel (its 16-byte form was measured slower there for its occupancy: profiles/seg_loss.txt, section 4).
// Every access is bounded by V.  Channel dispatch, base pointers, alignment rule, softmax exponentials and block tails: voxel_loss.hpp.
#include "voxel_loss.hpp"

namespace {

constexpr int FVPB = 4096;  // voxels per forward block (one partial each)
constexpr int BVPB = 256;   // voxels per backward block: one per thread

template <int C, bool SIG>
__device__ __forceinline__ void probs(const float (&z)[C], float (&p)[C]) {
    if constexpr (SIG) {
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] = 1.f / (1.f + expf(-z[c]));
    } else {
        float mx;
        const float inv = 1.f / softmax_exp<C>(z, p, mx);
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] *= inv;
    }
}

// one voxel's share of the sum; t[] (HAUSDORFF only) holds the target of each channel
template <int C, bool SIG>
__device__ __forceinline__ float fwd_voxel(const float (&z)[C], const float (&t)[C], const float (&a)[C], int kind, int c0) {
    float p[C], s = 0.f;
    probs<C, SIG>(z, p);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (c < c0) continue;
        if (kind == UNETR_DISTLOSS_BOUNDARY) {
            s += p[c] * a[c];
        } else {
            const float d = p[c] - t[c];
            s += d * d * a[c];
        }
    }
    return s;
}

// grid (ceil(V / FVPB), B); part[b * gridDim.x + blockIdx.x]
template <int C, bool SIG>
__global__ void __launch_bounds__(256)
distloss_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ target, const float* __restrict__ field, long V, int kind,
                    int c0, float* __restrict__ part) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const long v0 = (long)blockIdx.x * FVPB, v1 = std::min<long>(V, v0 + FVPB);
    const float* lg = item_channels<C>(logits, b, V);
    const float* fd = item_channels<C>(field, b, V);
    const bool need_t = kind == UNETR_DISTLOSS_HAUSDORFF;      // the boundary loss never reads the target
    const float* tg = need_t ? item_target<C, SIG>(target, b, V) : nullptr;
    float acc = 0.f;
    // its own walk: a third tensor, read for the included channels only, and a target that only one of the two kinds reads
    if (vec4_ok(V, logits, field, need_t ? target : nullptr)) {
        for (long v = v0 + 4 * threadIdx.x; v < v1; v += 1024) {
            f32x4 zv[C], av[C], tv[SIG ? C : 1];
#pragma unroll
            for (int c = 0; c < C; ++c) zv[c] = *(const f32x4*)(lg + (long)c * V + v);
#pragma unroll
            for (int c = 0; c < C; ++c) av[c] = c >= c0 ? *(const f32x4*)(fd + (long)c * V + v) : (f32x4){0.f, 0.f, 0.f, 0.f};
            if (need_t) {
                if constexpr (SIG) {
#pragma unroll
                    for (int c = 0; c < C; ++c) tv[c] = *(const f32x4*)(tg + (long)c * V + v);
                } else {
                    tv[0] = *(const f32x4*)(tg + v);
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float z[C], a[C], t[C];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    z[c] = zv[c][e]; a[c] = av[c][e];
                    t[c] = !need_t ? 0.f : SIG ? tv[SIG ? c : 0][e] : ((int)tv[0][e] == c ? 1.f : 0.f);
                }
                acc += fwd_voxel<C, SIG>(z, t, a, kind, c0);
            }
        }
    } else {
        for (long v = v0 + threadIdx.x; v < v1; v += 256) {
            float z[C], a[C], t[C];
            const int lab = need_t && !SIG ? (int)tg[v] : -1;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                z[c] = lg[(long)c * V + v];
                a[c] = c >= c0 ? fd[(long)c * V + v] : 0.f;
                t[c] = !need_t ? 0.f : SIG ? tg[(long)c * V + v] : (lab == c ? 1.f : 0.f);
            }
            acc += fwd_voxel<C, SIG>(z, t, a, kind, c0);
        }
    }
    block_wave_sums<1>(&acc, red);
    if (threadIdx.x == 0) part[(long)b * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

constexpr int FIN_THREADS = 1024, FIN_WAVES = FIN_THREADS / 64;

// one block: the partials in double, thread t takes t, t + 1024, ... in order, then the shuffle tree and the waves in order
__global__ void __launch_bounds__(FIN_THREADS)
distloss_final_kernel(const float* __restrict__ part, long npart, const float* __restrict__ weight, double count, float* __restrict__ out) {
    __shared__ double sh[FIN_WAVES];
    double s = 0.0;
    for (long i = threadIdx.x; i < npart; i += FIN_THREADS) s += (double)part[i];
    block_wave_sums<1>(&s, sh);
    if (threadIdx.x == 0) {
        s = 0.0;
        for (int w = 0; w < FIN_WAVES; ++w) s += sh[w];
        out[0] = (float)((double)weight[0] * s / count);
    }
}

// grid (ceil(V / BVPB), B); dlogits = *dloss * w / N * dL/dz, every element written
template <int C, bool SIG>
__global__ void __launch_bounds__(256)
distloss_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ target, const float* __restrict__ field,
                    const float* __restrict__ weight, const float* __restrict__ dloss, float inv_count, float* __restrict__ dlogits, long V,
                    int kind, int c0) {
    const int b = blockIdx.y;
    const long v = (long)blockIdx.x * BVPB + threadIdx.x;
    if (v >= V) return;
    const float* lg = item_channels<C>(logits, b, V);
    const float* fd = item_channels<C>(field, b, V);
    float* dl = item_channels<C>(dlogits, b, V);
    const float sc = (dloss ? *dloss : 1.f) * weight[0] * inv_count;
    float z[C], p[C], a[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        z[c] = lg[(long)c * V + v];
        a[c] = c >= c0 ? fd[(long)c * V + v] : 0.f;
    }
    probs<C, SIG>(z, p);
    if (kind == UNETR_DISTLOSS_HAUSDORFF) {
        const float* tg = item_target<C, SIG>(target, b, V);
        const int lab = SIG ? -1 : (int)tg[v];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float t = c < c0 ? 0.f : SIG ? tg[(long)c * V + v] : (lab == c ? 1.f : 0.f);
            a[c] = c >= c0 ? 2.f * (p[c] - t) * a[c] : 0.f;
        }
    }
    if constexpr (SIG) {
#pragma unroll
        for (int c = 0; c < C; ++c) dl[(long)c * V + v] = sc * (a[c] * p[c] * (1.f - p[c]));
    } else {
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) dot += p[c] * a[c];
#pragma unroll
        for (int c = 0; c < C; ++c) dl[(long)c * V + v] = sc * (p[c] * (a[c] - dot));
    }
}

int check_desc(const unetr_distloss_desc* d) {
    if (int rc = check_voxel_desc(d)) return rc;
    if (d->kind != UNETR_DISTLOSS_BOUNDARY && d->kind != UNETR_DISTLOSS_HAUSDORFF) return UNETR_ERR_ARG;
    if (!d->include_background && d->C == 1) return UNETR_ERR_ARG;
    return UNETR_OK;
}

double mean_count(const unetr_distloss_desc* d) {
    return (double)d->B * (double)(d->C - (d->include_background ? 0 : 1)) * (double)d->V;
}

}  // namespace

extern "C" size_t unetr_distloss_workspace_bytes(const unetr_distloss_desc* d) {
    if (check_desc(d) != UNETR_OK) return 0;
    return (size_t)d->B * cdiv(d->V, FVPB) * sizeof(float);
}

extern "C" int unetr_distloss_fwd(const unetr_distloss_desc* d, const float* logits, const float* target, const float* field,
                                  const float* weight, float* out, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_desc(d)) return rc;
    if (!logits || !field || !weight || !out || (d->kind == UNETR_DISTLOSS_HAUSDORFF && !target)) return UNETR_ERR_ARG;
    if (!ws || ((uintptr_t)ws & 15) || unetr_distloss_workspace_bytes(d) > ws_bytes) return UNETR_ERR_WORKSPACE;
    const int B = d->B, nchunk = cdiv(d->V, FVPB), kind = d->kind, c0 = d->include_background ? 0 : 1;
    const long V = d->V;
    float* part = (float*)ws;
    hipStream_t st = (hipStream_t)stream;
    VOXEL_DISPATCH(d->C, d->multilabel, hipLaunchKernelGGL((distloss_fwd_kernel<CC, SIG>), dim3(nchunk, B), dim3(256), 0, st, logits, target,
                                                           field, V, kind, c0, part));
    hipLaunchKernelGGL(distloss_final_kernel, dim3(1), dim3(FIN_THREADS), 0, st, part, (long)B * nchunk, weight, mean_count(d), out);
    return unetr_check_launch();
}

extern "C" int unetr_distloss_bwd(const unetr_distloss_desc* d, const float* logits, const float* target, const float* field,
                                  const float* weight, const float* dloss, float* dlogits, void* stream) {
    if (int rc = check_desc(d)) return rc;
    if (!logits || !field || !weight || !dlogits || (d->kind == UNETR_DISTLOSS_HAUSDORFF && !target)) return UNETR_ERR_ARG;
    const int B = d->B, nblk = cdiv(d->V, BVPB), kind = d->kind, c0 = d->include_background ? 0 : 1;
    const long V = d->V;
    const float inv_count = (float)(1.0 / mean_count(d));
    hipStream_t st = (hipStream_t)stream;
    VOXEL_DISPATCH(d->C, d->multilabel, hipLaunchKernelGGL((distloss_bwd_kernel<CC, SIG>), dim3(nblk, B), dim3(256), 0, st, logits, target,
                                                           field, weight, dloss, inv_count, dlogits, V, kind, c0));
    return unetr_check_launch();
}
