// DiceCELoss(to_onehot_y=True, softmax=True) forward + backward (unetr_segmentation_3d.py:404; MONAI 0.6.0
// defaults: include_background, squared_pred=False, jaccard=False, batch=False, reduction="mean",
// smooth_nr = smooth_dr = 1e-5, lambda_dice = lambda_ce = 1).
//
//   p = softmax(logits, 1);  y = one_hot(label)
//   per (b,c): I = sum p*y, G = sum y, Pp = sum p over the volume
//   dice = mean_{b,c} [1 - (2I + nr) / (G + Pp + dr)];  ce = mean_{b,v} -log p[b, label, v];  loss = dice + ce
//
// SIG mode = DiceCELoss(to_onehot_y=False, sigmoid=True) on a multi-label float target [B,C,*spatial]
// (unetr_segmentation_3d.py:477-482, the 4-channel MR task): the Dice term uses p = sigmoid(logits) against the target
// as given; the CE term is MONAI 0.6.0's DiceCELoss.ce with equal channel counts -- softmax cross entropy of the raw
// logits against argmax_c(target) (first maximal channel, torch.argmax's rule).
//
// HBM-bound: one pass over logits+label for the forward (fixed-order partial buffers -> reproducible), one
// pass for the backward that recomputes the softmax and writes dlogits.  Channel dispatch, base pointers, alignment rule, target
// decode and softmax exponentials: voxel_loss.hpp.
#include <algorithm>
#include "voxel_loss.hpp"

namespace {

constexpr int LVPB = 4096;  // voxels per block

template <int C, bool SIG>
__global__ void __launch_bounds__(256)
dicece_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ label, long V, float* __restrict__ part) {
    // part: [B][nchunk][3*C + 1]  (I[c], Pp[c], G[c], ce_sum)
    __shared__ float red[4][3 * C + 1];
    const int b = blockIdx.y;
    const long v0 = (long)blockIdx.x * LVPB, v1 = std::min<long>(V, v0 + LVPB);
    const float* lg = item_channels<C>(logits, b, V);
    const float* lb = item_target<C, SIG>(label, b, V);
    float accI[C], accP[C], accG[C], ce = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { accI[c] = 0.f; accP[c] = 0.f; accG[c] = 0.f; }
    // softmax / one-hot form on whole 4-voxel groups: one 16-byte load per channel and for the labels, all of an iteration's loads
    // in flight together (one voxel per iteration was 16 dependent memory round trips per thread: 19 us for 35 MB)
    if (!SIG && vec4_ok(V, logits, label)) {
        for (long v = v0 + 4 * threadIdx.x; v < v1; v += 1024) {      // (LVPB and V are multiples of 4: whole groups)
            f32x4 zv[C];
#pragma unroll
            for (int c = 0; c < C; ++c) zv[c] = *(const f32x4*)(lg + (long)c * V + v);
            const f32x4 lv = *(const f32x4*)(lb + v);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float z[C], mx;
#pragma unroll
                for (int c = 0; c < C; ++c) z[c] = zv[c][e];
                const float inv = 1.f / softmax_exp<C>(z, z, mx);
                const int lab = (int)lv[e];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    float p = z[c] * inv;
                    accP[c] += p;
                    if (c == lab) { accI[c] += p; accG[c] += 1.f; ce -= logf(p); }
                }
            }
        }
    } else
    for (long v = v0 + threadIdx.x; v < v1; v += 256) {
        float x[C], z[C], mx;
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] = lg[(long)c * V + v];
        const float inv = 1.f / softmax_exp<C>(x, z, mx);
        if constexpr (SIG) {
            float t[C];
#pragma unroll
            for (int c = 0; c < C; ++c) t[c] = lb[(long)c * V + v];
            const int lab = mask_argmax<C>(t);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float sg = 1.f / (1.f + expf(-x[c]));
                accP[c] += sg; accI[c] += sg * t[c]; accG[c] += t[c];
                if (c == lab) ce -= logf(z[c] * inv);
            }
        } else {
            const int lab = (int)lb[v];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float p = z[c] * inv;
                accP[c] += p;
                if (c == lab) { accI[c] += p; accG[c] += 1.f; ce -= logf(p); }
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float a = wave_sum(accI[c]), p = wave_sum(accP[c]), g = wave_sum(accG[c]);
        if (lane == 0) { red[wave][c] = a; red[wave][C + c] = p; red[wave][2 * C + c] = g; }
    }
    ce = wave_sum(ce);
    if (lane == 0) red[wave][3 * C] = ce;
    __syncthreads();
    if (threadIdx.x < 3 * C + 1)
        part[((long)b * gridDim.x + blockIdx.x) * (3 * C + 1) + threadIdx.x] =
            red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// single block: reduce partials in double (fixed order: lanes stride over the chunks, shuffle tree), emit loss terms and the
// Dice gradient coefficients.  One wave per (b, c) -- eight threads walking 216 chunks each serially cost 30 us.
// coef[(b*C+c)*2+0] = dDice/dp coefficient on y:  -2/(B*C*den);  [+1] = constant term: (2I+nr)/(B*C*den^2)
__global__ void __launch_bounds__(256)
dicece_final_kernel(const float* __restrict__ part, int B, int C, int nchunk, long V, float nr, float dr,
                    float* __restrict__ out, float* __restrict__ coef) {
    __shared__ double sdice[4];
    __shared__ double sce[4];
    const int stride = 3 * C + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double dice_acc = 0.0, ce_acc = 0.0;
    for (int i = wave; i < B * C; i += 4) {
        const int b = i / C, c = i - b * C;
        double I = 0.0, Pp = 0.0, G = 0.0;
        for (int k = lane; k < nchunk; k += 64) {
            const float* p = part + ((long)b * nchunk + k) * stride;
            I += (double)p[c]; Pp += (double)p[C + c]; G += (double)p[2 * C + c];
        }
        I = wave_sum_d(I); Pp = wave_sum_d(Pp); G = wave_sum_d(G);
        const double den = G + Pp + (double)dr, num = 2.0 * I + (double)nr;
        dice_acc += 1.0 - num / den;
        if (lane == 0) {
            coef[2 * i] = (float)(-2.0 / ((double)(B * C) * den));
            coef[2 * i + 1] = (float)(num / ((double)(B * C) * den * den));
        }
    }
    for (int i = threadIdx.x; i < B * nchunk; i += 256) ce_acc += (double)part[(long)i * stride + 3 * C];
    ce_acc = wave_sum_d(ce_acc);
    if (lane == 0) { sdice[wave] = dice_acc; sce[wave] = ce_acc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double dice = (sdice[0] + sdice[1] + sdice[2] + sdice[3]) / (double)(B * C);
        const double ce = (sce[0] + sce[1] + sce[2] + sce[3]) / ((double)B * (double)V);
        out[0] = (float)(dice + ce); out[1] = (float)dice; out[2] = (float)ce;
    }
}

template <int C, bool SIG>
__global__ void __launch_bounds__(256)
dicece_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ label, const float* __restrict__ coef,
                  const float* __restrict__ dloss, float* __restrict__ dlogits, int B, long V) {
    const float up = dloss ? *dloss : 1.f;
    const float ce_scale = 1.f / ((float)B * (float)V);
    const long total = (long)B * V;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / V); const long v = i - (long)b * V;
        const float* lg = item_channels<C>(logits, b, V);
        const float* lb = item_target<C, SIG>(label, b, V);
        float* dl = item_channels<C>(dlogits, b, V);
        const float* cf = coef + (long)b * C * 2;
        float x[C], z[C], mx;
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] = lg[(long)c * V + v];
        const float inv = 1.f / softmax_exp<C>(x, z, mx);
        if constexpr (SIG) {
            float t[C];
#pragma unroll
            for (int c = 0; c < C; ++c) t[c] = lb[(long)c * V + v];
            const int lab = mask_argmax<C>(t);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float sg = 1.f / (1.f + expf(-x[c]));
                const float dz = (cf[2 * c] * t[c] + cf[2 * c + 1]) * sg * (1.f - sg) + (z[c] * inv - (c == lab ? 1.f : 0.f)) * ce_scale;
                dl[(long)c * V + v] = up * dz;
            }
            continue;
        }
        const int lab = (int)lb[v];
        float gp[C], dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            z[c] *= inv;                                   // p_c
            gp[c] = (c == lab ? cf[2 * c] : 0.f) + cf[2 * c + 1];      // dDice/dp_c
            dot += z[c] * gp[c];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float dz = z[c] * (gp[c] - dot) + (z[c] - (c == lab ? 1.f : 0.f)) * ce_scale;
            dl[(long)c * V + v] = up * dz;
        }
    }
}

}  // namespace

extern "C" int unetr_dicece_fwd(const float* logits, const float* label, int B, int C, long V, int sigmoid_multilabel,
                                float smooth_nr, float smooth_dr, float* out, float* coef, float* ws, size_t ws_bytes,
                                void* stream) {
    if (!logits || !label || !out || !coef) return UNETR_ERR_ARG;
    if (int rc = check_voxel_dims(B, C, V)) return rc;
    int nchunk = cdiv(V, LVPB);
    if (!ws || (size_t)B * nchunk * (3 * C + 1) * sizeof(float) > ws_bytes) return UNETR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    VOXEL_DISPATCH(C, sigmoid_multilabel,
                   hipLaunchKernelGGL((dicece_fwd_kernel<CC, SIG>), dim3(nchunk, B), dim3(256), 0, st, logits, label, V, ws));
    hipLaunchKernelGGL(dicece_final_kernel, dim3(1), dim3(256), 0, st, ws, B, C, nchunk, V, smooth_nr, smooth_dr, out, coef);
    return unetr_check_launch();
}

extern "C" int unetr_dicece_bwd(const float* logits, const float* label, const float* coef, const float* dloss,
                                float* dlogits, int B, int C, long V, int sigmoid_multilabel, void* stream) {
    if (!logits || !label || !coef || !dlogits) return UNETR_ERR_ARG;
    if (int rc = check_voxel_dims(B, C, V, false)) return rc;      // (one grid dimension over B*V: no cap on B)
    hipStream_t st = (hipStream_t)stream;
    long total = (long)B * V;
    int blocks = (int)std::max<long>(1, std::min<long>((total + 255) / 256, 8192));
    VOXEL_DISPATCH(C, sigmoid_multilabel, hipLaunchKernelGGL((dicece_bwd_kernel<CC, SIG>), dim3(blocks), dim3(256), 0, st, logits,
                                                             label, coef, dloss, dlogits, B, V));
    return unetr_check_launch();
}
