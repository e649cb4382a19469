// Dense exact Euclidean distance transform of N = B*C binary masks [D,H,W] and the distance fields of the distance-map losses
// (configuration: unetr_edt_desc, include/unetr_hip.h).  scipy.ndimage.distance_transform_edt's convention: the distance of every
// voxel to the nearest voxel where the mask is 0, 0 on those voxels themselves; +inf everywhere for a mask without a zero.
//
// Separable, three launches per call (per group of batch items that fits the caller's workspace):
//   edt_xpass_kernel       derives the masks of one x-line for all C channels of an item from the input form (float / byte mask,
//                          class ids, softmax or sigmoid of logits > 0.5: no one-hot tensor exists anywhere), keeps them as bit
//                          words in LDS and writes g(x) = (s_x * steps to the nearest zero along the line)^2, +inf for a line
//                          without one.  One wave per line, adjacent x in adjacent lanes.
//   edt_colpass_kernel<1>  exact min-plus  f(i) = min_j g(j) + (s_y (i - j))^2  along y, in place: tiles of COLS adjacent x-columns,
//                          whole lines in LDS (the layout of hd_colpass_kernel in metrics.hip).
//   edt_colpass_kernel<0>  the same along z, and the field assembly on the way out: sqrt, sign, offset, power, accumulation.
//
// The fields (signed, unsigned) need the distance to the nearest foreground voxel outside the object (d_fg) and to the nearest
// background voxel inside it (d_bg).  At every voxel exactly one of the two is non-zero, so the passes along x and y carry TWO
// fields (0: to the nearest zero of the mask, 1: to the nearest one) and the pass along z evaluates only the one the voxel needs:
// the voxel is inside the object exactly when field 0 is non-zero at it.  A mask that is empty or fills the volume has one field
// +inf everywhere; the assembled field is 0 there (no boundary in view), never inf - inf.
//
// Arithmetic: float32 throughout, every term (s * k)^2 as __fmul_rn(t, t) of t = __fmul_rn(s, k), sums as __fadd_rn in the order
// (x + y) + z, no contraction.  With unit spacing all of it is exact integer arithmetic below 3 * 511^2 < 2^24.
//
// The min-plus walks outwards from i, k = 0, 1, 2, ...: candidates i - k and i + k, and it stops at the first k whose own term
// (s k)^2 reaches the best value so far -- g >= 0 and rounding is monotone, so no later candidate can be smaller.  The result is
// the exact minimum over the whole line; on masks with boundaries in view the walk is a few steps long.  It is confined to the
// finite range [jlo, jhi] of the line (found by a scan from both ends) and starts at the range when i lies outside it, so a line
// that is +inf throughout -- every line of a class that is absent from the crop -- costs one scan and no walk.
//
// Every access is bounded: x < W, the line index < its extent, the item < the group's count.
#include "common.hpp"

namespace {

constexpr int EDT_MAXN = 512;                 // largest extent of an axis
constexpr int EDT_MAXC = 16;                  // largest channel count (the loss family's cap)
constexpr int EDT_XWORDS = EDT_MAXN / 64;     // 64-bit words of one x-line's mask
constexpr int EDT_COLS = 32;                  // x-columns per tile of the column passes ...
constexpr int EDT_COLS_TALL = 16;             // ... and of the z pass with two fields when D > EDT_TALL (64 KiB of LDS either way)
constexpr int EDT_TALL = 256;

struct EdtGeom {
    int C, D, H, W;
    float sz, sy, sx;
};
struct EdtOut {
    int field, squared, accumulate;
    float u, alpha;
};

__device__ __forceinline__ float edt_inf() { return __builtin_huge_valf(); }

// bit c of the result: the mask of channel c holds a one at voxel v of item b
template <int FORM>
__device__ __forceinline__ uint32_t member_bits(const void* __restrict__ src, long b, int C, long V, long v) {
    uint32_t bits = 0;
    if constexpr (FORM == UNETR_EDT_FORM_MASK) {
        const float* p = (const float*)src + b * C * V + v;
        for (int c = 0; c < C; ++c) bits |= (p[(long)c * V] != 0.f ? 1u : 0u) << c;
    } else if constexpr (FORM == UNETR_EDT_FORM_MASK_U8) {
        const uint8_t* p = (const uint8_t*)src + b * C * V + v;
        for (int c = 0; c < C; ++c) bits |= (p[(long)c * V] != 0 ? 1u : 0u) << c;
    } else if constexpr (FORM == UNETR_EDT_FORM_CLASS_IDS) {
        const int lab = (int)((const float*)src)[b * V + v];
        bits = lab >= 0 && lab < C ? 1u << lab : 0u;
    } else {
        const float* p = (const float*)src + b * C * V + v;
        float z[EDT_MAXC];
#pragma unroll
        for (int c = 0; c < EDT_MAXC; ++c) z[c] = c < C ? p[(long)c * V] : -3.0e38f;
        if constexpr (FORM == UNETR_EDT_FORM_SOFTMAX) {        // the probabilities as the loss kernels compute them
            float mx = -3.0e38f, se = 0.f;
#pragma unroll
            for (int c = 0; c < EDT_MAXC; ++c) mx = fmaxf(mx, z[c]);
#pragma unroll
            for (int c = 0; c < EDT_MAXC; ++c) { z[c] = c < C ? expf(z[c] - mx) : 0.f; se += z[c]; }
            const float inv = 1.f / se;
#pragma unroll
            for (int c = 0; c < EDT_MAXC; ++c) bits |= (c < C && z[c] * inv > 0.5f ? 1u : 0u) << c;
        } else {
#pragma unroll
            for (int c = 0; c < EDT_MAXC; ++c) bits |= (c < C && 1.f / (1.f + expf(-z[c])) > 0.5f ? 1u : 0u) << c;
        }
    }
    return bits;
}

// steps from x to the nearest set bit of a line's words (ones = false: of their complement inside [0, W)); -1 when there is none
__device__ __forceinline__ int nearest_bit(const uint64_t* __restrict__ w, int nw, int W, int x, bool ones) {
    const int k0 = x >> 6, b0 = x & 63;
    int best = -1;
    for (int k = k0; k >= 0; --k) {
        const int left = W - k * 64;
        const uint64_t vm = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
        uint64_t m = (ones ? w[k] : ~w[k]) & vm;
        if (k == k0) m &= ~0ull >> (63 - b0);
        if (m) { best = x - (k * 64 + 63 - __clzll((long long)m)); break; }
    }
    for (int k = k0; k < nw; ++k) {
        const int left = W - k * 64;
        const uint64_t vm = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
        uint64_t m = (ones ? w[k] : ~w[k]) & vm;
        if (k == k0) m &= ~0ull << b0;
        if (m) {
            const int d = k * 64 + __ffsll((unsigned long long)m) - 1 - x;
            best = best < 0 || d < best ? d : best;
            break;
        }
    }
    return best;
}

__device__ __forceinline__ float sq_term(float s, int k) {
    const float t = __fmul_rn(s, (float)k);
    return __fmul_rn(t, t);
}

// grid (ceil(D*H / 4), items of the group); wave w of a block takes x-line 4 * blockIdx.x + w of item b0 + blockIdx.y.
// ws: [NF][items * C][D*H*W] floats, fstride = items * C * D*H*W.
template <int FORM, int NF>
__global__ void __launch_bounds__(256)
edt_xpass_kernel(const void* __restrict__ src, int b0, EdtGeom g, float* __restrict__ ws, long fstride) {
    __shared__ uint64_t ones[4][EDT_MAXC][EDT_XWORDS];      // bit x of word x / 64: the mask of channel c is one at x (0 past W)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C = g.C, W = g.W, nw = (W + 63) >> 6;
    const long nlines = (long)g.D * g.H, V = nlines * W;
    const long l = (long)blockIdx.x * 4 + wave;
    const bool valid = l < nlines;
    if (valid) {
        for (int k = 0; k < nw; ++k) {
            const int x = k * 64 + lane;
            const uint32_t bits = x < W ? member_bits<FORM>(src, (long)b0 + blockIdx.y, C, V, l * W + x) : 0u;
            for (int c = 0; c < C; ++c) {
                const uint64_t m = __ballot((bits >> c) & 1u);
                if (lane == 0) ones[wave][c][k] = m;
            }
        }
    }
    __syncthreads();
    if (!valid) return;
    for (int c = 0; c < C; ++c) {
        float* o = ws + ((long)blockIdx.y * C + c) * V + l * W;
        for (int x = lane; x < W; x += 64) {
            const int d0 = nearest_bit(ones[wave][c], nw, W, x, false);
            o[x] = d0 < 0 ? edt_inf() : sq_term(g.sx, d0);
            if constexpr (NF == 2) {
                const int d1 = nearest_bit(ones[wave][c], nw, W, x, true);
                o[fstride + x] = d1 < 0 ? edt_inf() : sq_term(g.sx, d1);
            }
        }
    }
}

// [jlo, jhi]: the first and the last finite element of a line in LDS; jlo = n (> jhi) for a line that is +inf throughout
template <int COLS>
__device__ __forceinline__ void finite_range(const float* __restrict__ t, int n, int& jlo, int& jhi) {
    jlo = 0;
    jhi = n - 1;
    while (jlo < n && t[jlo * COLS] == edt_inf()) ++jlo;
    while (jhi > jlo && t[jhi * COLS] == edt_inf()) --jhi;
}

// exact min over j of t[j * COLS] + (s (i - j))^2, outwards from i (see the head of the file), over the finite range of the line
template <int COLS>
__device__ __forceinline__ float min_plus(const float* __restrict__ t, int i, int jlo, int jhi, float s) {
    float best = t[i * COLS];
    if (jlo > jhi) return best;
    for (int k = i < jlo ? jlo - i : i > jhi ? i - jhi : 1;; ++k) {
        const int lo = i - k, hi = i + k;
        if (lo < jlo && hi > jhi) break;
        const float q = sq_term(s, k);
        if (q >= best) break;
        if (lo >= jlo) best = fminf(best, __fadd_rn(t[lo * COLS], q));
        if (hi <= jhi) best = fminf(best, __fadd_rn(t[hi * COLS], q));
    }
    return best;
}

// AXIS 1: lines along y, one tile = (z, COLS x-columns) of one mask and one field (blockIdx.z), in place in ws.
// AXIS 0: lines along z, one tile = (y, COLS x-columns) of one mask with all NF fields; writes the assembled field to out.
// grid (tiles per mask, masks of the group, AXIS 1 ? NF : 1); dynamic LDS: (AXIS 1 ? 1 : NF) * n * COLS floats.
template <int AXIS, int NF, int COLS>
__global__ void __launch_bounds__(256)
edt_colpass_kernel(float* __restrict__ ws, long fstride, EdtGeom g, EdtOut eo, float* __restrict__ out) {
    extern __shared__ float tile[];
    constexpr int ROWS = 256 / COLS, NL = AXIS == 1 ? 1 : NF;
    const int n = AXIS == 1 ? g.H : g.D, W = g.W;
    const int nxc = (W + COLS - 1) / COLS;
    const int col = threadIdx.x & (COLS - 1), rg = threadIdx.x / COLS;
    const int o = blockIdx.x / nxc, x = (blockIdx.x - o * nxc) * COLS + col;
    const long V = (long)g.D * g.H * W;
    const long sj = AXIS == 1 ? W : (long)g.H * W;
    const long base = (long)blockIdx.y * V + (AXIS == 1 ? (long)o * g.H * W : (long)o * W) + x;
    float* f = ws + (AXIS == 1 ? (long)blockIdx.z * fstride : 0);
    const float s = AXIS == 1 ? g.sy : g.sz;
#pragma unroll
    for (int k = 0; k < NL; ++k)
        for (int j = rg; j < n; j += ROWS) tile[(k * n + j) * COLS + col] = x < W ? f[k * fstride + base + j * sj] : edt_inf();
    __syncthreads();
    if (x >= W) return;
    int jlo[NL], jhi[NL];
#pragma unroll
    for (int k = 0; k < NL; ++k) finite_range<COLS>(tile + col + k * n * COLS, n, jlo[k], jhi[k]);
    if (AXIS == 1 && jlo[0] > jhi[0]) return;                           // +inf throughout, and so it stays
    for (int i = rg; i < n; i += ROWS) {
        if constexpr (AXIS == 1) {
            f[base + i * sj] = min_plus<COLS>(tile + col, i, jlo[0], jhi[0], s);
        } else {
            const bool inside = tile[i * COLS + col] != 0.f;            // the mask is one here: field 0 is the distance to its zeros
            const int k = NF == 2 && !inside ? 1 : 0;
            const float d2 = min_plus<COLS>(tile + col + k * n * COLS, i, k ? jlo[NL - 1] : jlo[0], k ? jhi[NL - 1] : jhi[0], s);
            float r;
            if (eo.field == UNETR_EDT_FIELD_DISTANCE) {
                r = eo.squared ? d2 : sqrtf(d2);
            } else if (d2 == edt_inf()) {
                r = 0.f;                                                  // the mask is empty or full: no boundary in view
            } else if (eo.field == UNETR_EDT_FIELD_SIGNED) {
                const float d = sqrtf(d2);
                r = inside ? -(d - eo.u) : d;
            } else {
                r = eo.alpha == 2.f ? d2 : eo.alpha == 1.f ? sqrtf(d2) : powf(sqrtf(d2), eo.alpha);
            }
            float* q = out + base + i * sj;
            *q = eo.accumulate ? *q + r : r;
        }
    }
}

int check_desc(const unetr_edt_desc* d) {
    if (!d || d->B <= 0 || d->D <= 0 || d->H <= 0 || d->W <= 0) return UNETR_ERR_ARG;
    if (d->C < 1 || d->C > EDT_MAXC || d->D > EDT_MAXN || d->H > EDT_MAXN || d->W > EDT_MAXN) return UNETR_ERR_UNSUPPORTED;
    if (d->form < UNETR_EDT_FORM_MASK || d->form > UNETR_EDT_FORM_SIGMOID) return UNETR_ERR_ARG;
    if (d->field < UNETR_EDT_FIELD_DISTANCE || d->field > UNETR_EDT_FIELD_UNSIGNED) return UNETR_ERR_ARG;
    if (d->has_spacing)
        for (int a = 0; a < 3; ++a)
            if (!(d->spacing[a] > 0.f) || !(d->spacing[a] < 3.0e38f)) return UNETR_ERR_ARG;
    if (d->field == UNETR_EDT_FIELD_UNSIGNED && !(d->alpha > 0.f)) return UNETR_ERR_ARG;
    if (d->accumulate && d->field != UNETR_EDT_FIELD_UNSIGNED) return UNETR_ERR_ARG;
    return UNETR_OK;
}

size_t item_bytes(const unetr_edt_desc* d) {
    const size_t nf = d->field == UNETR_EDT_FIELD_DISTANCE ? 1 : 2;
    return nf * (size_t)d->C * d->D * d->H * d->W * sizeof(float);
}

template <int NF>
void launch_xpass(int form, dim3 grid, hipStream_t st, const void* src, int b0, EdtGeom g, float* ws, long fstride) {
#define EDT_X(F) hipLaunchKernelGGL((edt_xpass_kernel<F, NF>), grid, dim3(256), 0, st, src, b0, g, ws, fstride)
    switch (form) {
        case UNETR_EDT_FORM_MASK: EDT_X(UNETR_EDT_FORM_MASK); break;
        case UNETR_EDT_FORM_MASK_U8: EDT_X(UNETR_EDT_FORM_MASK_U8); break;
        case UNETR_EDT_FORM_CLASS_IDS: EDT_X(UNETR_EDT_FORM_CLASS_IDS); break;
        case UNETR_EDT_FORM_SOFTMAX: EDT_X(UNETR_EDT_FORM_SOFTMAX); break;
        default: EDT_X(UNETR_EDT_FORM_SIGMOID); break;
    }
#undef EDT_X
}

template <int NF>
void launch_group(const unetr_edt_desc* d, const void* src, float* out, float* ws, int b0, int nb, hipStream_t st) {
    const EdtGeom g{d->C, d->D, d->H, d->W, d->has_spacing ? d->spacing[0] : 1.f, d->has_spacing ? d->spacing[1] : 1.f,
                    d->has_spacing ? d->spacing[2] : 1.f};
    const EdtOut eo{d->field, d->squared, d->accumulate, d->has_spacing ? std::min(g.sz, std::min(g.sy, g.sx)) : 1.f, d->alpha};
    const long V = (long)d->D * d->H * d->W, fstride = (long)nb * d->C * V;
    const int masks = nb * d->C;
    launch_xpass<NF>(d->form, dim3(cdiv((long)d->D * d->H, 4), nb), st, src, b0, g, ws, fstride);
    if (d->H > 1)         // (a line of one element is its own minimum)
        hipLaunchKernelGGL((edt_colpass_kernel<1, NF, EDT_COLS>), dim3(d->D * cdiv(d->W, EDT_COLS), masks, NF), dim3(256),
                           (size_t)d->H * EDT_COLS * sizeof(float), st, ws, fstride, g, eo, (float*)nullptr);
    float* o = out + (long)b0 * d->C * V;
    if (NF == 2 && d->D > EDT_TALL)
        hipLaunchKernelGGL((edt_colpass_kernel<0, NF, EDT_COLS_TALL>), dim3(d->H * cdiv(d->W, EDT_COLS_TALL), masks), dim3(256),
                           (size_t)NF * d->D * EDT_COLS_TALL * sizeof(float), st, ws, fstride, g, eo, o);
    else
        hipLaunchKernelGGL((edt_colpass_kernel<0, NF, EDT_COLS>), dim3(d->H * cdiv(d->W, EDT_COLS), masks), dim3(256),
                           (size_t)NF * d->D * EDT_COLS * sizeof(float), st, ws, fstride, g, eo, o);
}

}  // namespace

extern "C" size_t unetr_edt_workspace_bytes(const unetr_edt_desc* d) {
    if (check_desc(d) != UNETR_OK) return 0;
    return item_bytes(d) * (size_t)d->B;
}

extern "C" int unetr_edt(const unetr_edt_desc* d, const void* src, float* out, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_desc(d)) return rc;
    if (!src || !out) return UNETR_ERR_ARG;
    const size_t per = item_bytes(d);
    if (!ws || ((uintptr_t)ws & 15) || ws_bytes < per) return UNETR_ERR_WORKSPACE;
    // items per group: what the workspace holds, and at most 65535 masks in a grid dimension
    const int nb_max = (int)std::min<size_t>(std::min<size_t>(ws_bytes / per, (size_t)d->B), (size_t)(65535 / d->C));
    hipStream_t st = (hipStream_t)stream;
    for (int b0 = 0; b0 < d->B; b0 += nb_max) {
        const int nb = std::min(nb_max, d->B - b0);
        if (d->field == UNETR_EDT_FIELD_DISTANCE) launch_group<1>(d, src, out, (float*)ws, b0, nb, st);
        else launch_group<2>(d, src, out, (float*)ws, b0, nb, st);
    }
    return unetr_check_launch();
}
