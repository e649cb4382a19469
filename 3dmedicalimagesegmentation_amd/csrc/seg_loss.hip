// Segmentation loss family: loss = lambda_region * R + lambda_voxel * X  (configuration: unetr_segloss_desc, include/unetr_hip.h)
//
//   R in {none, Dice, Jaccard, Tversky, generalized Dice}   on p = softmax(logits, 1) vs one_hot(label)   (one-hot mode)
//                                                           or p = sigmoid(logits)    vs the float mask    (multilabel mode)
//   X in {none, cross entropy, sigmoid focal}               on the raw logits
//
// Every region variant is a function of three per-(b,c) sums over the volume,
//   I = sum p*y,   P = sum p (p^2 with squared_pred),   G = sum y (y^2 with squared_pred),
// and its derivative with respect to one probability is  dR/dp_c(v) = a*y + b*p + k  with three per-(b,c) numbers.  So the
// family shares ONE forward pass (fixed-order partial buffers -> reproducible, no float atomics), one single-block finalize in
// double that turns the sums into (loss, R, X) and the coefficients, and ONE backward pass that recomputes the probabilities and
// writes dlogits.  The forward pass moves whole 4-voxel groups as 16-byte loads per channel in both modes (its scalar loop takes
// over when V % 4 != 0 or a pointer is not 16-byte aligned); the backward pass runs one voxel per thread.  Every access is bounded
// by V.
//
// ignore_index (one-hot mode): a voxel whose label equals it adds to no sum and gets a zero gradient; the voxel means then
// divide by what G counted, so the finalize needs no further partial.
//
// Channel dispatch, base pointers, alignment rule, target decode, softmax exponentials and the finalize's block tail: voxel_loss.hpp.
#include <algorithm>
#include "voxel_loss.hpp"

namespace {

constexpr int FVPB = 4096;  // voxels per forward block (one partial row each)
constexpr int BVPB = 256;   // voxels per backward block: one per thread

struct SegCfg {
    const float* cw;      // class weights [C] or null
    float gamma;
    int squared, voxel, c0, has_ignore, ignore;      // c0: first channel of the region term and of the focal mean
};

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// sigmoid focal value of one element: exp(gamma * logsigmoid(-z(2t-1))) * bce(z, t).  BIN: t is 0 or 1 (a one-hot target), so
// |z(2t-1)| = |z| and the two log1p(exp(-|.|)) are one
template <bool BIN>
__device__ __forceinline__ float focal_val(float z, float t, float gamma) {
    const float l = log1pf(expf(-fabsf(z)));
    const float bce = fmaxf(z, 0.f) - z * t + l;
    if (gamma == 0.f) return bce;
    const float s = -z * (2.f * t - 1.f);
    const float ls = fminf(s, 0.f) - (BIN ? l : log1pf(expf(-fabsf(s))));
    return expf(gamma * ls) * bce;
}

// d focal_val / dz = mod * [(sigmoid(z) - t) - gamma * (1 - sigmoid(s)) * (2t-1) * bce],  mod = exp(gamma * logsigmoid(s))
template <bool BIN>
__device__ __forceinline__ float focal_grad(float z, float t, float gamma) {
    const float e = expf(-fabsf(z));
    const float sg = (z >= 0.f ? 1.f : e) / (1.f + e);
    float g = sg - t;
    if (gamma != 0.f) {
        const float l = log1pf(e);
        const float bce = fmaxf(z, 0.f) - z * t + l;
        const float m = 2.f * t - 1.f, s = -z * m;
        const float es = BIN ? e : expf(-fabsf(s));
        const float ls = fminf(s, 0.f) - (BIN ? l : log1pf(es));
        const float one_minus_sgs = (s >= 0.f ? es : 1.f) / (1.f + es);
        g = expf(gamma * ls) * (g - gamma * one_minus_sgs * m * bce);
    }
    return g;
}

template <int C>
struct SegAcc {
    float I[C], P[C], G[C], x;
};

template <int C, bool SIG>
__device__ __forceinline__ void seg_fwd_voxel(const float (&z)[C], const float (&t)[C], int lab, const SegCfg& cfg, const float (&w)[C],
                                              SegAcc<C>& acc) {
    float e[C], mx = -3.0e38f, se = 0.f;
    if (!SIG || cfg.voxel == UNETR_SEGLOSS_VOXEL_CE) se = softmax_exp<C>(z, e, mx);
    const float inv = 1.f / se;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float p = SIG ? sigmoidf_(z[c]) : e[c] * inv;
        acc.I[c] += p * t[c];
        acc.P[c] += cfg.squared ? p * p : p;
        acc.G[c] += cfg.squared ? t[c] * t[c] : t[c];
    }
    if (cfg.voxel == UNETR_SEGLOSS_VOXEL_CE) {
        float zl = 0.f, wl = 1.f;
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (c == lab) zl = z[c];
        if (cfg.cw) {
#pragma unroll
            for (int c = 0; c < C; ++c)
                if (c == lab) wl = w[c];
        }
        acc.x += wl * (logf(se) - (zl - mx));       // -log softmax(z)[lab]
    } else if (cfg.voxel == UNETR_SEGLOSS_VOXEL_FOCAL) {
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (c >= cfg.c0) acc.x += w[c] * focal_val<!SIG>(z[c], t[c], cfg.gamma);
    }
}

template <int C, bool SIG>
__global__ void __launch_bounds__(256)
segloss_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ label, long V, SegCfg cfg, float* __restrict__ part) {
    // part: [B][nchunk][3*C + 1]  (I[c], P[c], G[c], voxel-term sum)
    __shared__ float red[4][3 * C + 1];
    const int b = blockIdx.y;
    const long v0 = (long)blockIdx.x * FVPB, v1 = std::min<long>(V, v0 + FVPB);
    SegAcc<C> acc;
    float w[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { acc.I[c] = 0.f; acc.P[c] = 0.f; acc.G[c] = 0.f; w[c] = cfg.cw ? cfg.cw[c] : 1.f; }
    acc.x = 0.f;
    const float* lg = item_channels<C>(logits, b, V);
    const float* lb = item_target<C, SIG>(label, b, V);
    if (vec4_ok(V, logits, label)) {
        // whole 4-voxel groups (FVPB and V are multiples of 4): one 16-byte load per channel of the logits and of the mask, or one
        // for the labels, all of an iteration's loads in flight together
        for (long v = v0 + 4 * threadIdx.x; v < v1; v += 1024) {
            f32x4 zv[C], tv[SIG ? C : 1];
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
                float z[C], t[C];
                int lab;
#pragma unroll
                for (int c = 0; c < C; ++c) z[c] = zv[c][e];
                if constexpr (SIG) {
#pragma unroll
                    for (int c = 0; c < C; ++c) t[c] = tv[c][e];
                    lab = mask_argmax<C>(t);
                } else {
                    lab = (int)tv[0][e];
                    if (cfg.has_ignore && lab == cfg.ignore) continue;
                    onehot_target<C>(lab, t);
                }
                seg_fwd_voxel<C, SIG>(z, t, lab, cfg, w, acc);
            }
        }
    } else {
        for (long v = v0 + threadIdx.x; v < v1; v += 256) {
            float z[C], t[C];
            int lab;
            if constexpr (SIG) {
#pragma unroll
                for (int c = 0; c < C; ++c) t[c] = lb[(long)c * V + v];
                lab = mask_argmax<C>(t);
            } else {
                lab = (int)lb[v];
                if (cfg.has_ignore && lab == cfg.ignore) continue;
                onehot_target<C>(lab, t);
            }
#pragma unroll
            for (int c = 0; c < C; ++c) z[c] = lg[(long)c * V + v];
            seg_fwd_voxel<C, SIG>(z, t, lab, cfg, w, acc);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float a = wave_sum(acc.I[c]), p = wave_sum(acc.P[c]), g = wave_sum(acc.G[c]);
        if (lane == 0) { red[wave][c] = a; red[wave][C + c] = p; red[wave][2 * C + c] = g; }
    }
    const float x = wave_sum(acc.x);
    if (lane == 0) red[wave][3 * C] = x;
    __syncthreads();
    if (threadIdx.x < 3 * C + 1)
        part[((long)b * gridDim.x + blockIdx.x) * (3 * C + 1) + threadIdx.x] =
            red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

constexpr int FIN_THREADS = 1024, FIN_WAVES = FIN_THREADS / 64;

constexpr int FIN_LDS_SUMS = 3 * 256;      // per-(b,c) sums stay in LDS up to B*C = 256, else in the workspace

// Single block.  Phase 1: one wave per (b, c) reduces the partial rows in double (fixed order: lanes stride over the chunks,
// shuffle tree) into sums[(b*C+c)*3 + {I,P,G}].  Phase 2: one wave per item (a batch item, or the whole batch with batch=1), lane c
// on channel c, evaluates the region term from those sums and writes coef[(b*C+c)*3 + {a,b,k}] (lambda_region and the mean folded
// in); coef[B*C*3] is the factor of the voxel term's gradient (lambda_voxel / its denominator).
__global__ void __launch_bounds__(FIN_THREADS)
segloss_final_kernel(const float* __restrict__ part, double* sums, unetr_segloss_desc d, int nchunk,
                     float* __restrict__ out, float* __restrict__ coef) {
    __shared__ double sh[FIN_WAVES][4];
    __shared__ double lds_sums[FIN_LDS_SUMS];
    const int B = d.B, C = d.C, stride = 3 * C + 1;
    if (3 * B * C <= FIN_LDS_SUMS) sums = lds_sums;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = wave; i < B * C; i += FIN_WAVES) {
        const int b = i / C, c = i - b * C;
        double I = 0.0, P = 0.0, G = 0.0;
        for (int k = lane; k < nchunk; k += 64) {
            const float* p = part + ((long)b * nchunk + k) * stride;
            I += (double)p[c]; P += (double)p[C + c]; G += (double)p[2 * C + c];
        }
        I = wave_sum_d(I); P = wave_sum_d(P); G = wave_sum_d(G);
        if (lane == 0) { sums[3 * i] = I; sums[3 * i + 1] = P; sums[3 * i + 2] = G; }
    }
    double xs = 0.0;
    for (long i = threadIdx.x; i < (long)B * nchunk; i += FIN_THREADS) xs += (double)part[i * stride + 3 * C];
    __syncthreads();                                     // sums[] is complete

    const int c0 = d.include_background ? 0 : 1;
    const int nitem = d.batch ? 1 : B, nb = d.batch ? B : 1;
    const double nr = (double)d.smooth_nr, dr = (double)d.smooth_dr, al = (double)d.alpha, be = (double)d.beta;
    const bool gdl = d.region == UNETR_SEGLOSS_REGION_GDL;
    const double scale = d.region == UNETR_SEGLOSS_REGION_NONE ? 0.0
                                                                : (double)d.lambda_region / ((double)nitem * (gdl ? 1.0 : (double)(C - c0)));
    double racc = 0.0;
    for (int it = wave; it < nitem; it += FIN_WAVES) {
        const int b0 = d.batch ? 0 : it, c = lane;
        const bool on = d.region != UNETR_SEGLOSS_REGION_NONE && c >= c0 && c < C;      // this lane's channel is part of the term
        double I = 0.0, P = 0.0, G = 0.0;
        if (on)
            for (int b = b0; b < b0 + nb; ++b) {
                const double* q = sums + ((long)b * C + c) * 3;
                I += q[0]; P += q[1]; G += q[2];
            }
        double a = 0.0, k = 0.0, f = 0.0;                // d f/dp = a y + k dP/dp
        if (gdl) {
            double wc = d.w_type == UNETR_SEGLOSS_W_SQUARE ? 1.0 / (G * G) : d.w_type == UNETR_SEGLOSS_W_SIMPLE ? 1.0 / G : 1.0;
            const bool fin = on && isfinite(wc);
            const double wmax = wave_max_d(fin ? wc : 0.0);      // largest finite weight of the item (0 when there is none)
            wc = !on ? 0.0 : fin ? wc : wmax;
            const double num = nr + wave_sum_d(2.0 * wc * I), den = dr + wave_sum_d(wc * (G + P));
            if (lane == c0) f = 1.0 - num / den;              // one value per item
            a = -2.0 * wc / den; k = num * wc / (den * den);
        } else if (on) {
            double num, den;
            if (d.region == UNETR_SEGLOSS_REGION_DICE) {
                num = 2.0 * I + nr; den = G + P + dr;
                a = -2.0 / den; k = num / (den * den);
            } else if (d.region == UNETR_SEGLOSS_REGION_JACCARD) {
                num = 2.0 * I + nr; den = 2.0 * (G + P - I) + dr;
                a = -2.0 / den - 2.0 * num / (den * den); k = 2.0 * num / (den * den);
            } else {                                      // Tversky
                num = I + nr; den = I + al * (P - I) + be * (G - I) + dr;
                a = -1.0 / den + num * (1.0 - al - be) / (den * den); k = num * al / (den * den);
            }
            f = 1.0 - num / den;
        }
        racc += f;
        if (c < C) {
            // dP/dp = 1, or 2p with squared_pred: the constant then moves to the coefficient of p
            const float fa = on ? (float)(a * scale) : 0.f, fk = on ? (float)(k * scale * (d.squared_pred ? 2.0 : 1.0)) : 0.f;
            for (int b = b0; b < b0 + nb; ++b) {
                float* q = coef + ((long)b * C + c) * 3;
                q[0] = fa; q[1] = d.squared_pred ? fk : 0.f; q[2] = d.squared_pred ? 0.f : fk;
            }
        }
    }
    // denominators of the voxel means from G (all channels, the background included): the weighted and the plain count of the
    // voxels that contributed
    double wd = 0.0, cnt = 0.0;
    for (int i = threadIdx.x; i < B * C; i += FIN_THREADS) {
        const double G = sums[3 * i + 2];
        wd += (d.class_weight ? (double)d.class_weight[i % C] : 1.0) * G; cnt += G;
    }
    const double mine[4] = {racc, wd, cnt, xs};
    block_wave_sums<4>(mine, &sh[0][0]);
    if (threadIdx.x == 0) {
        racc = wd = cnt = xs = 0.0;
        for (int w = 0; w < FIN_WAVES; ++w) { racc += sh[w][0]; wd += sh[w][1]; cnt += sh[w][2]; xs += sh[w][3]; }
        const double R = d.region == UNETR_SEGLOSS_REGION_NONE ? 0.0 : racc / ((double)nitem * (gdl ? 1.0 : (double)(C - c0)));
        const double all = (double)B * (double)d.V;
        const bool counted = !d.multilabel && (d.has_ignore || d.class_weight);      // else every voxel counts once: B*V exactly
        double den = 1.0;
        if (d.voxel == UNETR_SEGLOSS_VOXEL_CE) den = counted ? wd : all;
        if (d.voxel == UNETR_SEGLOSS_VOXEL_FOCAL) den = (!d.multilabel && d.has_ignore ? cnt : all) * (double)(C - c0);
        const double X = d.voxel == UNETR_SEGLOSS_VOXEL_NONE ? 0.0 : xs / den;
        out[0] = (float)((double)d.lambda_region * R + (double)d.lambda_voxel * X); out[1] = (float)R; out[2] = (float)X;
        coef[(long)B * C * 3] = d.voxel == UNETR_SEGLOSS_VOXEL_NONE ? 0.f : (float)((double)d.lambda_voxel / den);
    }
}

// gradient of one voxel: z[] holds the logits on entry and up * dloss/dlogits on return
template <int C, bool SIG>
__device__ __forceinline__ void seg_bwd_voxel(float (&z)[C], const float (&t)[C], int lab, const SegCfg& cfg, const float (&w)[C],
                                              const float (&ca)[C], const float (&cb)[C], const float (&ck)[C], float vs, float up) {
    float sm[C], dz[C];
    if (!SIG || cfg.voxel == UNETR_SEGLOSS_VOXEL_CE) {
        float mx;
        const float inv = 1.f / softmax_exp<C>(z, sm, mx);
#pragma unroll
        for (int c = 0; c < C; ++c) sm[c] *= inv;
    }
    if constexpr (SIG) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float sg = sigmoidf_(z[c]);
            const float g = cfg.squared ? ca[c] * t[c] + cb[c] * sg : ca[c] * t[c] + ck[c];      // dR/dp_c: b != 0 only with squared_pred, and then k = 0
            dz[c] = g * sg * (1.f - sg);
        }
    } else {
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            dz[c] = cfg.squared ? ca[c] * t[c] + cb[c] * sm[c] : ca[c] * t[c] + ck[c];      // dR/dp_c: b != 0 only with squared_pred, and then k = 0
            dot += sm[c] * dz[c];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) dz[c] = sm[c] * (dz[c] - dot);
    }
    if (cfg.voxel == UNETR_SEGLOSS_VOXEL_CE) {
        float wl = 1.f;
        if (cfg.cw) {
#pragma unroll
            for (int c = 0; c < C; ++c)
                if (c == lab) wl = w[c];
        }
        const float vw = vs * wl;
#pragma unroll
        for (int c = 0; c < C; ++c) dz[c] += vw * (sm[c] - (c == lab ? 1.f : 0.f));
    } else if (cfg.voxel == UNETR_SEGLOSS_VOXEL_FOCAL) {
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (c >= cfg.c0) dz[c] += vs * w[c] * focal_grad<!SIG>(z[c], t[c], cfg.gamma);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) z[c] = up * dz[c];
}

// One voxel per thread, scalar accesses, as dicece_bwd_kernel: at B*V of a training batch this pass sits at the bandwidth the chip
// gives either way, and the 16-byte form (four voxels per thread: C or 2C vectors of inputs live at once) was built and measured
// slower for its low occupancy -- profiles/seg_loss.txt, section 4.
template <int C, bool SIG>
__global__ void __launch_bounds__(256)
segloss_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ label, const float* __restrict__ coef,
                   const float* __restrict__ dloss, float* __restrict__ dlogits, int B, long V, SegCfg cfg) {
    const int b = blockIdx.y;
    const long v = (long)blockIdx.x * BVPB + threadIdx.x;
    if (v >= V) return;
    const float* lg = item_channels<C>(logits, b, V);
    const float* lb = item_target<C, SIG>(label, b, V);
    float* dl = item_channels<C>(dlogits, b, V);
    const float up = dloss ? *dloss : 1.f;
    const float vs = coef[(long)B * C * 3];
    float w[C], ca[C], cb[C], ck[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float* q = coef + ((long)b * C + c) * 3;
        ca[c] = q[0]; cb[c] = q[1]; ck[c] = q[2];
        w[c] = cfg.cw ? cfg.cw[c] : 1.f;
    }
    float z[C], t[C];
    int lab;
    bool valid = true;
    if constexpr (SIG) {
#pragma unroll
        for (int c = 0; c < C; ++c) t[c] = lb[(long)c * V + v];
        lab = mask_argmax<C>(t);
    } else {
        lab = (int)lb[v];
        valid = !(cfg.has_ignore && lab == cfg.ignore);
        onehot_target<C>(lab, t);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) z[c] = lg[(long)c * V + v];
    if (valid) seg_bwd_voxel<C, SIG>(z, t, lab, cfg, w, ca, cb, ck, vs, up);
#pragma unroll
    for (int c = 0; c < C; ++c) dl[(long)c * V + v] = valid ? z[c] : 0.f;
}

int check_desc(const unetr_segloss_desc* d) {
    if (int rc = check_voxel_desc(d)) return rc;
    if (d->region < UNETR_SEGLOSS_REGION_NONE || d->region > UNETR_SEGLOSS_REGION_GDL || d->voxel < UNETR_SEGLOSS_VOXEL_NONE ||
        d->voxel > UNETR_SEGLOSS_VOXEL_FOCAL || d->w_type < UNETR_SEGLOSS_W_SQUARE || d->w_type > UNETR_SEGLOSS_W_UNIFORM)
        return UNETR_ERR_ARG;
    if (d->region == UNETR_SEGLOSS_REGION_NONE && d->voxel == UNETR_SEGLOSS_VOXEL_NONE) return UNETR_ERR_ARG;
    if (!d->include_background && d->C == 1) return UNETR_ERR_ARG;
    if (d->squared_pred && (d->region == UNETR_SEGLOSS_REGION_TVERSKY || d->region == UNETR_SEGLOSS_REGION_GDL)) return UNETR_ERR_UNSUPPORTED;
    if (d->multilabel && (d->has_ignore || (d->class_weight && d->voxel == UNETR_SEGLOSS_VOXEL_CE))) return UNETR_ERR_UNSUPPORTED;
    return UNETR_OK;
}

SegCfg make_cfg(const unetr_segloss_desc* d) {
    SegCfg cfg;
    cfg.cw = d->voxel == UNETR_SEGLOSS_VOXEL_NONE ? nullptr : d->class_weight;
    cfg.gamma = d->gamma;
    cfg.squared = d->squared_pred != 0;
    cfg.voxel = d->voxel;
    cfg.c0 = d->include_background ? 0 : 1;
    cfg.has_ignore = !d->multilabel && d->has_ignore;
    cfg.ignore = d->ignore_index;
    return cfg;
}

size_t part_bytes(const unetr_segloss_desc* d) {      // the partial rows, rounded up so that the doubles behind them are aligned
    const size_t n = (size_t)d->B * cdiv(d->V, FVPB) * (3 * d->C + 1) * sizeof(float);
    return (n + 15) & ~(size_t)15;
}

}  // namespace

extern "C" size_t unetr_segloss_workspace_bytes(const unetr_segloss_desc* d) {
    if (check_desc(d) != UNETR_OK) return 0;
    return part_bytes(d) + (size_t)d->B * d->C * 3 * sizeof(double);
}

extern "C" int unetr_segloss_fwd(const unetr_segloss_desc* d, const float* logits, const float* label, float* out, float* coef,
                                 void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_desc(d)) return rc;
    if (!logits || !label || !out || !coef) return UNETR_ERR_ARG;
    if (!ws || ((uintptr_t)ws & 15) || unetr_segloss_workspace_bytes(d) > ws_bytes) return UNETR_ERR_WORKSPACE;
    const int B = d->B, nchunk = cdiv(d->V, FVPB);
    const long V = d->V;
    const SegCfg cfg = make_cfg(d);
    float* part = (float*)ws;
    double* sums = (double*)((char*)ws + part_bytes(d));
    hipStream_t st = (hipStream_t)stream;
    VOXEL_DISPATCH(d->C, d->multilabel,
                   hipLaunchKernelGGL((segloss_fwd_kernel<CC, SIG>), dim3(nchunk, B), dim3(256), 0, st, logits, label, V, cfg, part));
    hipLaunchKernelGGL(segloss_final_kernel, dim3(1), dim3(FIN_THREADS), 0, st, part, sums, *d, nchunk, out, coef);
    return unetr_check_launch();
}

extern "C" int unetr_segloss_bwd(const unetr_segloss_desc* d, const float* logits, const float* label, const float* coef,
                                 const float* dloss, float* dlogits, void* stream) {
    if (int rc = check_desc(d)) return rc;
    if (!logits || !label || !coef || !dlogits) return UNETR_ERR_ARG;
    const int B = d->B, nblk = cdiv(d->V, BVPB);
    const long V = d->V;
    const SegCfg cfg = make_cfg(d);
    hipStream_t st = (hipStream_t)stream;
    VOXEL_DISPATCH(d->C, d->multilabel, hipLaunchKernelGGL((segloss_bwd_kernel<CC, SIG>), dim3(nblk, B), dim3(256), 0, st, logits, label,
                                                           coef, dloss, dlogits, B, V, cfg));
    return unetr_check_launch();
}
