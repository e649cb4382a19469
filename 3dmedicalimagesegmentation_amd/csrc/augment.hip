// GPU-resident random crop sampling and augmentation: the per-step random part of the reference's
// training transforms (unetr_segmentation_3d.py:322-476, unetr_ranking_pretraining_3d.py:346-444), MONAI 0.6.0 semantics as
// restated in tests/augment_ref.py.
//
// VolumeCache.add (setup, may synchronise):
//   aug_prep_kernel      ScaleIntensityRanged (same float32 operations as MONAI, no contraction) in place, the bounding box
//                        of any_c(image > 0) by integer atomics, a flag for label values that are not integers in 0..255
//   aug_crop_kernel      copies the foreground box: image float32, label uint8
//   aug_count_kernel     per chunk of AUG_CHUNK voxels the number of foreground / background voxels of map_binary_to_indices
//   aug_scan_kernel      exclusive scan of the chunk counts (one workgroup) and the two totals
//   aug_scatter_kernel   ordered compaction: each chunk again, AUG_CHUNK / 256 rounds of ballot + prefix, ascending ravel order
// RandCropAugment.__call__ (per step: launches only, no host sync, no allocation):
//   aug_sample_kernel    one workgroup: Philox4x64-10 draws, crop centres, the params table, counter and cursor advance;
//                        <true> also draws the rotation / zoom of each sample and writes the affine table
//   aug_gather_kernel    every output voxel back through rot90^k, the flips and the corner to its source voxel; C image
//                        channels (+ shift) and L label bytes; with normalize also fp64 partial sums per workgroup;
//                        <., true> takes the samples its affine table flags through the matrix to a position between
//                        voxels of the whole volume: trilinear image, nearest label, border padding (aug_affine_voxel)
//   aug_norm_kernel      fixed-order reduction of the partials and (x - mean) / std over the nonzero voxels
#include <algorithm>
#include <math.h>
#include "common.hpp"
#include "../../include/unetr_hip.h"

namespace {

constexpr int AUG_CHUNK = 4096;       // voxels per workgroup of the count / scatter passes (16 rounds of 256)
constexpr int AUG_VPT = 8;            // output voxels per thread of the gather (one workgroup = 2048 voxels of one sample)
constexpr int AUG_TILE = 256 * AUG_VPT;
constexpr int AUG_MAXC = 8;           // image channels / label channels
constexpr int AUG_MAXS = 512;         // crop extent per axis
constexpr int AUG_NORM_WG = 64;       // workgroups per (sample, channel) of the normalize pass
constexpr int AUG_ROW = 8;            // ints per params row: vol, z0, y0, x0, flip mask, k, shift flag, offset (float bits)
constexpr int AUG_VCOLS = 12;         // int64 per volume table row: img, lbl, fg, nfg, bg, nbg, C, L, D, H, W, 0
constexpr int AUG_AROW = 16;          // floats per affine row: flag, angle about axis 0, 1, 2, zoom of axis 0, 1, 2, M [3][3] row-major
constexpr int AUG_BR0 = 8, AUG_BR1 = 16, AUG_BR2 = 16;   // output brick of one workgroup on a flagged sample (= AUG_TILE voxels)
constexpr int AUG_MAXDIM_AFFINE = 1 << 24;               // extent up to which a float32 coordinate names every voxel
static_assert(AUG_BR0 == AUG_VPT && AUG_BR1 * AUG_BR2 == 256, "one brick plane per round of the workgroup");

// ---------------------------------------------------------------- Philox4x64-10 (Salmon et al. 2011; numpy.random.Philox)
struct Ph4 { unsigned long long v[4]; };

__device__ __forceinline__ Ph4 philox4x64(Ph4 c, unsigned long long k0, unsigned long long k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B97F4A7C15ull; k1 += 0xBB67AE8584CAA73Bull; }
        const unsigned long long a = 0xD2E7470EE14C6C93ull, b = 0xCA5A826395121157ull;
        const unsigned long long hi0 = __umul64hi(a, c.v[0]), lo0 = a * c.v[0];
        const unsigned long long hi1 = __umul64hi(b, c.v[2]), lo1 = b * c.v[2];
        Ph4 o;
        o.v[0] = hi1 ^ c.v[1] ^ k0; o.v[1] = lo1; o.v[2] = hi0 ^ c.v[3] ^ k1; o.v[3] = lo0;
        c = o;
    }
    return c;
}
// block j of sample s in call n: counter (n, s, j, 0), key (seed, 0)
__device__ __forceinline__ Ph4 aug_block(unsigned long long seed, unsigned long long n, int s, int j) {
    Ph4 c; c.v[0] = n; c.v[1] = (unsigned long long)s; c.v[2] = (unsigned long long)j; c.v[3] = 0ull;
    return philox4x64(c, seed, 0ull);
}
__device__ __forceinline__ double u01(unsigned long long w) { return (double)(w >> 11) * 0x1.0p-53; }
__device__ __forceinline__ long long randint(unsigned long long w, unsigned long long n) { return (long long)__umul64hi(w, n); }

// monai.transforms.utils.correct_crop_centers (0.6.0) for one axis
__device__ __forceinline__ long long correct_center(long long c, int S, long long dim) {
    const long long vs = S / 2;
    long long ve = (long long)floor((double)(dim + 1) - (double)S / 2.0);
    if (vs == ve) ve += 1;
    if (c < vs) c = vs;
    if (c >= ve) c = ve - 1;
    return c;
}

// ---------------------------------------------------------------- add(): scale / clip, box, label check
__global__ void __launch_bounds__(256)
aug_prep_kernel(float* __restrict__ img, const float* __restrict__ lbl, int C, int L, int D, int H, int W, int scale_mode,
                float a_min, float a_range, float b_range, float b_min, float b_max, int do_box, int* __restrict__ box,
                int* __restrict__ flag) {
#pragma clang fp contract(off)
    const long V = (long)D * H * W;
    __shared__ int sbox[6];
    __shared__ int sflag;
    if (threadIdx.x < 6) sbox[threadIdx.x] = threadIdx.x < 3 ? 0x7fffffff : -1;
    if (threadIdx.x == 0) sflag = 0;
    __syncthreads();
    int bz0 = 0x7fffffff, by0 = 0x7fffffff, bx0 = 0x7fffffff, bz1 = -1, by1 = -1, bx1 = -1, bad = 0;
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long)gridDim.x * 256) {
        bool any = false;
        for (int c = 0; c < C; ++c) {
            float x = img[(long)c * V + v];
            if (scale_mode == 1) {
                x = (x - a_min) / a_range;
                x = x * b_range + b_min;
                x = fminf(fmaxf(x, b_min), b_max);        // np.clip
                img[(long)c * V + v] = x;
            } else if (scale_mode == 2) {                  // a_max == a_min: MONAI returns img - a_min
                x = x - a_min;
                img[(long)c * V + v] = x;
            }
            any |= x > 0.f;
        }
        for (int l = 0; l < L; ++l) {
            const float t = lbl[(long)l * V + v];
            if (!(t >= 0.f && t <= 255.f && t == floorf(t))) bad = 1;
        }
        if (do_box && any) {
            const int x = (int)(v % W), y = (int)((v / W) % H), z = (int)(v / ((long)W * H));
            bz0 = min(bz0, z); by0 = min(by0, y); bx0 = min(bx0, x);
            bz1 = max(bz1, z); by1 = max(by1, y); bx1 = max(bx1, x);
        }
    }
    if (do_box) {
        atomicMin(&sbox[0], bz0); atomicMin(&sbox[1], by0); atomicMin(&sbox[2], bx0);
        atomicMax(&sbox[3], bz1); atomicMax(&sbox[4], by1); atomicMax(&sbox[5], bx1);
    }
    if (bad) atomicOr(&sflag, 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (do_box) {
            atomicMin(&box[0], sbox[0]); atomicMin(&box[1], sbox[1]); atomicMin(&box[2], sbox[2]);
            atomicMax(&box[3], sbox[3]); atomicMax(&box[4], sbox[4]); atomicMax(&box[5], sbox[5]);
        }
        if (sflag) atomicOr(flag, 1);
    }
}

// grid (ceil(w / 256), h, d * (C + L)): one row of the box per workgroup slice
__global__ void __launch_bounds__(256)
aug_crop_kernel(const float* __restrict__ img, const float* __restrict__ lbl, int C, int L, int D, int H, int W, int z0, int y0,
                int x0, int d, int h, int w, float* __restrict__ oimg, uint8_t* __restrict__ olbl) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y;
    const int z = blockIdx.z % d, ch = blockIdx.z / d;
    if (x >= w) return;
    const long src = ((long)(z0 + z) * H + (y0 + y)) * W + (x0 + x);
    const long dst = ((long)z * h + y) * w + x;
    const long V = (long)D * H * W, v = (long)d * h * w;
    if (ch < C) oimg[ch * v + dst] = img[ch * V + src];
    else olbl[(ch - C) * v + dst] = (uint8_t)lbl[(ch - C) * V + src];
}

// ---------------------------------------------------------------- add(): map_binary_to_indices as an ordered compaction
__device__ __forceinline__ void fg_bg(const float* __restrict__ img, const uint8_t* __restrict__ lbl, int C, int L, long V,
                                      float thr, long v, bool& fg, bool& bg) {
    fg = false;
    for (int l = 0; l < L; ++l) fg |= lbl[(long)l * V + v] != 0;
    bool any = false;
    for (int c = 0; c < C; ++c) any |= img[(long)c * V + v] > thr;
    bg = !fg && any;
}

// ws (ints): [cnt_fg nblk][cnt_bg nblk][off_fg nblk][off_bg nblk][total_fg, total_bg]
__global__ void __launch_bounds__(256)
aug_count_kernel(const float* __restrict__ img, const uint8_t* __restrict__ lbl, int C, int L, long V, float thr,
                 int* __restrict__ ws, int nblk) {
    __shared__ int red[2][4];
    int nf = 0, nb = 0;
    const long base = (long)blockIdx.x * AUG_CHUNK;
    for (int i = 0; i < AUG_CHUNK / 256; ++i) {
        const long v = base + i * 256 + threadIdx.x;
        if (v >= V) break;
        bool f, b;
        fg_bg(img, lbl, C, L, V, thr, v, f, b);
        nf += f; nb += b;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { nf += __shfl_xor(nf, o, 64); nb += __shfl_xor(nb, o, 64); }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wv] = nf; red[1][wv] = nb; }
    __syncthreads();
    if (threadIdx.x == 0) {
        ws[blockIdx.x] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        ws[nblk + blockIdx.x] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    }
}

// one workgroup of 1024 threads: thread t scans a contiguous segment, thread 0 scans the 1024 segment sums
__global__ void __launch_bounds__(1024) aug_scan_kernel(int* __restrict__ ws, int nblk) {
    __shared__ int seg[2][1024];
    const int per = (nblk + 1023) / 1024;
    const int b0 = min(nblk, (int)threadIdx.x * per), b1 = min(nblk, b0 + per);
    for (int k = 0; k < 2; ++k) {
        int s = 0;
        for (int b = b0; b < b1; ++b) s += ws[k * nblk + b];
        seg[k][threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int k = threadIdx.x;
        int run = 0;
        for (int t = 0; t < 1024; ++t) { const int s = seg[k][t]; seg[k][t] = run; run += s; }
        ws[4 * nblk + k] = run;
    }
    __syncthreads();
    for (int k = 0; k < 2; ++k) {
        int run = seg[k][threadIdx.x];
        for (int b = b0; b < b1; ++b) { ws[(2 + k) * nblk + b] = run; run += ws[k * nblk + b]; }
    }
}

__global__ void __launch_bounds__(256)
aug_scatter_kernel(const float* __restrict__ img, const uint8_t* __restrict__ lbl, int C, int L, long V, float thr,
                   const int* __restrict__ ws, int nblk, int* __restrict__ fgi, int* __restrict__ bgi) {
    __shared__ int wtot[2][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    int of = ws[2 * nblk + blockIdx.x], ob = ws[3 * nblk + blockIdx.x];
    const long base = (long)blockIdx.x * AUG_CHUNK;
    for (int i = 0; i < AUG_CHUNK / 256; ++i) {
        const long v = base + i * 256 + threadIdx.x;
        bool f = false, b = false;
        if (v < V) fg_bg(img, lbl, C, L, V, thr, v, f, b);
        const unsigned long long mf = __ballot(f), mb = __ballot(b);
        if (lane == 0) { wtot[0][wv] = __popcll(mf); wtot[1][wv] = __popcll(mb); }
        __syncthreads();
        int pf = of, pb = ob;
        for (int k = 0; k < wv; ++k) { pf += wtot[0][k]; pb += wtot[1][k]; }
        if (f) fgi[pf + __popcll(mf & below)] = (int)v;
        if (b) bgi[pb + __popcll(mb & below)] = (int)v;
        of += wtot[0][0] + wtot[0][1] + wtot[0][2] + wtot[0][3];
        ob += wtot[1][0] + wtot[1][1] + wtot[1][2] + wtot[1][3];
        __syncthreads();
    }
}

// ---------------------------------------------------------------- per call: sampler
// state (int64): [call counter, cursor, len(order), 0]
// AFFINE: block 3 word 0 flags the sample, words 1..3 are the angles about axes 0..2, block 4 words 0..2 the zooms (word 0
// for all three unless zoom_per_axis); blocks 0..2 are drawn as without it.  Angles and zooms are lo + (hi - lo) * u in
// double, stored as float32; M = (R0 . R1) . R2 . diag(1 / z) in double from the STORED values, rounded once.
template <bool AFFINE>
__global__ void __launch_bounds__(256)
aug_sample_kernel(UnetrAugDesc d, UnetrAugAffineDesc af, const long long* __restrict__ vols, int nvol,
                  const int* __restrict__ order, long long* __restrict__ state, int* __restrict__ params,
                  float* __restrict__ affine) {
#pragma clang fp contract(off)
    const unsigned long long n = (unsigned long long)state[0];
    const long long cursor = state[1];
    const long long norder = state[2] > 0 ? state[2] : 1;
    const int S[3] = {d.S0, d.S1, d.S2};
    for (int s = threadIdx.x; s < d.B; s += 256) {
        const int item = s / d.num_samples;
        int vol = order[(cursor + item) % norder];
        if (vol < 0 || vol >= nvol) vol = 0;
        const long long* t = vols + (long)vol * AUG_VCOLS;
        const long long dim[3] = {t[8], t[9], t[10]};
        const Ph4 w0 = aug_block(d.seed, n, s, 0), w1 = aug_block(d.seed, n, s, 1), w2 = aug_block(d.seed, n, s, 2);
        long long corner[3];
        if (d.sampling == 0) {                               // RandCropByPosNegLabeld
            const long long nfg = t[3], nbg = t[5];
            const double pr = nfg == 0 ? 0.0 : (nbg == 0 ? 1.0 : d.pos_ratio);
            const bool pos = u01(w0.v[0]) < pr;
            const long long len = pos ? nfg : nbg;
            const int* list = (const int*)(pos ? t[2] : t[4]);
            const long long idx = list[randint(w0.v[1], (unsigned long long)len)];
            const long long c[3] = {idx / (dim[1] * dim[2]), (idx / dim[2]) % dim[1], idx % dim[2]};
            for (int a = 0; a < 3; ++a) corner[a] = correct_center(c[a], S[a], dim[a]) - S[a] / 2;
        } else {                                             // RandSpatialCropSamplesd(random_size=False)
            for (int a = 0; a < 3; ++a) corner[a] = randint(w0.v[a], (unsigned long long)(dim[a] - S[a] + 1));
        }
        int flips = 0;
        for (int a = 0; a < 3; ++a) flips |= (u01(w1.v[a]) < d.flip_prob[a]) << a;
        const int k = u01(w1.v[3]) < d.rot90_prob ? (int)randint(w2.v[0], (unsigned long long)d.max_k) + 1 : 0;
        const int shift = u01(w2.v[1]) < d.shift_prob;
        const float off = shift ? (float)(d.shift_lo + (d.shift_hi - d.shift_lo) * u01(w2.v[2])) : 0.f;
        int* row = params + (long)s * AUG_ROW;
        row[0] = vol; row[1] = (int)corner[0]; row[2] = (int)corner[1]; row[3] = (int)corner[2];
        row[4] = flips; row[5] = k; row[6] = shift; row[7] = __float_as_int(off);
        if (AFFINE) {
            const Ph4 w3 = aug_block(d.seed, n, s, 3), w4 = aug_block(d.seed, n, s, 4);
            float* arow = affine + (long)s * AUG_AROW;
            const bool on = u01(w3.v[0]) < af.prob;
            float ang[3] = {0.f, 0.f, 0.f}, zm[3] = {1.f, 1.f, 1.f};
            float m[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
            if (on) {
                double c[3], sn[3], inv[3];
                for (int a = 0; a < 3; ++a) {
                    ang[a] = (float)(-af.rotate[a] + (af.rotate[a] - -af.rotate[a]) * u01(w3.v[1 + a]));
                    zm[a] = (float)(af.zoom_lo + (af.zoom_hi - af.zoom_lo) * u01(w4.v[af.zoom_per_axis ? a : 0]));
                    c[a] = cos((double)ang[a]); sn[a] = sin((double)ang[a]); inv[a] = 1.0 / (double)zm[a];
                }
                const double r0[3][3] = {{1.0, 0.0, 0.0}, {0.0, c[0], -sn[0]}, {0.0, sn[0], c[0]}};
                const double r1[3][3] = {{c[1], 0.0, sn[1]}, {0.0, 1.0, 0.0}, {-sn[1], 0.0, c[1]}};
                const double r2[3][3] = {{c[2], -sn[2], 0.0}, {sn[2], c[2], 0.0}, {0.0, 0.0, 1.0}};
                double t[3][3];
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j) t[i][j] = (r0[i][0] * r1[0][j] + r0[i][1] * r1[1][j]) + r0[i][2] * r1[2][j];
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j)
                        m[i * 3 + j] = (float)(((t[i][0] * r2[0][j] + t[i][1] * r2[1][j]) + t[i][2] * r2[2][j]) * inv[j]);
            }
            arow[0] = on ? 1.f : 0.f;
            for (int a = 0; a < 3; ++a) { arow[1 + a] = ang[a]; arow[4 + a] = zm[a]; }
            for (int j = 0; j < 9; ++j) arow[7 + j] = m[j];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        state[0] = (long long)(n + 1);
        state[1] = (cursor + d.B / d.num_samples) % norder;
    }
}

// ---------------------------------------------------------------- per call: gather (+ normalize partials)
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// crop position p of output voxel o: back through np.rot90(k, axes=(ra, rb)) (n = S[ra] = S[rb]), then the flips
__device__ __forceinline__ void aug_crop_pos(const int o[3], const int S[3], int k, int ra, int rb, int n, int flips, int p[3]) {
    p[0] = o[0]; p[1] = o[1]; p[2] = o[2];
    if (k == 1) { p[ra] = o[rb]; p[rb] = n - 1 - o[ra]; }
    else if (k == 2) { p[ra] = n - 1 - o[ra]; p[rb] = n - 1 - o[rb]; }
    else if (k == 3) { p[ra] = n - 1 - o[rb]; p[rb] = o[ra]; }
#pragma unroll
    for (int a = 0; a < 3; ++a) if (flips >> a & 1) p[a] = S[a] - 1 - p[a];
}

// The arithmetic of a flagged sample, float32 with no contraction, in the one order tests/augment_affine_ref.py restates:
//   q_a   = (float)p_a - half_a,  half_a = (float)(S_a - 1) * 0.5f,  centre_a = (float)c0_a + half_a
//   src_a = centre_a + ((M[a][0] * q0 + M[a][1] * q1) + M[a][2] * q2),  then clamped to [-1, dim_a]: whatever the matrix, the
//           conversion to int below stays in range, and with border padding a position that far outside reads the border voxel
//   f = floorf(src), t = src - f, i0 = clamp(f, 0, dim - 1), i1 = clamp(f + 1, 0, dim - 1)
//   image: lerp a + t * (b - a) along axis 2, then 1, then 0;  label: voxel clamp(floorf(src + 0.5f), 0, dim - 1)
struct AugTaps { long base[4]; int dx; float t[3]; long near; };     // base: (i0|i1 of axis 0, i0|i1 of axis 1) at i0 of axis 2

__device__ __forceinline__ AugTaps aug_affine_taps(const int p[3], const float* m, const float half[3], const float centre[3],
                                                   const int dims[3]) {
#pragma clang fp contract(off)
    const float q[3] = {(float)p[0] - half[0], (float)p[1] - half[1], (float)p[2] - half[2]};
    int i0[3], i1[3], nr[3];
    AugTaps tp;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float src = centre[a] + ((m[a * 3] * q[0] + m[a * 3 + 1] * q[1]) + m[a * 3 + 2] * q[2]);
        src = fminf(fmaxf(src, -1.f), (float)dims[a]);
        const float f = floorf(src);
        tp.t[a] = src - f;
        i0[a] = min(max((int)f, 0), dims[a] - 1);
        i1[a] = min(max((int)f + 1, 0), dims[a] - 1);
        nr[a] = min(max((int)floorf(src + 0.5f), 0), dims[a] - 1);
    }
    const long H = dims[1], W = dims[2];
    tp.base[0] = ((long)i0[0] * H + i0[1]) * W + i0[2];
    tp.base[1] = ((long)i0[0] * H + i1[1]) * W + i0[2];
    tp.base[2] = ((long)i1[0] * H + i0[1]) * W + i0[2];
    tp.base[3] = ((long)i1[0] * H + i1[1]) * W + i0[2];
    tp.dx = i1[2] - i0[2];
    tp.near = ((long)nr[0] * H + nr[1]) * W + nr[2];
    return tp;
}

__device__ __forceinline__ float aug_trilinear(const float* __restrict__ img, const AugTaps& tp) {
#pragma clang fp contract(off)
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float a = img[tp.base[j]], b = img[tp.base[j] + tp.dx];
        r[j] = a + tp.t[2] * (b - a);
    }
    const float u0 = r[0] + tp.t[1] * (r[1] - r[0]), u1 = r[2] + tp.t[1] * (r[3] - r[2]);
    return u0 + tp.t[0] * (u1 - u0);
}

// workgroups per sample of the affine gather: enough for the ravel tiles of an unflagged sample and the bricks of a flagged one
inline int aug_affine_blocks(const UnetrAugDesc* d) {
    const long V = (long)d->S0 * d->S1 * d->S2;
    return std::max(cdiv(V, AUG_TILE), cdiv(d->S0, AUG_BR0) * cdiv(d->S1, AUG_BR1) * cdiv(d->S2, AUG_BR2));
}

// grid (ceil(V / AUG_TILE), B); part: [B][C][gridDim.x][3] (count, sum, sum of squares over x != 0)
// AFFINE: grid (aug_affine_blocks, B).  A sample whose affine row is flagged is cut into bricks of AUG_BR0 x AUG_BR1 x AUG_BR2
// output voxels, one per workgroup, a 16 x 16 plane per round: the eight taps of neighbouring threads then share cache lines
// whatever the rotation.  An unflagged sample takes the integer path below, tile for tile as without AFFINE (uniform per
// workgroup), so it is written bit for bit as aug_gather_kernel<NORM, false> writes it.
template <bool NORM, bool AFFINE>
__global__ void __launch_bounds__(256)
aug_gather_kernel(UnetrAugDesc d, const long long* __restrict__ vols, int nvol, const int* __restrict__ params,
                  const float* __restrict__ affine, float* __restrict__ x, float* __restrict__ y, double* __restrict__ part) {
#pragma clang fp contract(off)
    const int s = blockIdx.y;
    const int* row = params + (long)s * AUG_ROW;
    const int vol = row[0];
    const int S[3] = {d.S0, d.S1, d.S2};
    const long V = (long)S[0] * S[1] * S[2];
    bool ok = vol >= 0 && vol < nvol;
    const long long* t = vols + (long)(ok ? vol : 0) * AUG_VCOLS;
    const int D = (int)t[8], H = (int)t[9], W = (int)t[10];
    const int c0[3] = {row[1], row[2], row[3]};
    const int dims[3] = {D, H, W};
    ok = ok && t[6] == d.C && t[7] == d.L;
    for (int a = 0; a < 3; ++a) ok = ok && c0[a] >= 0 && c0[a] + S[a] <= dims[a];
    const int flips = row[4], k = row[5] & 3, shift = row[6];
    const float off = __int_as_float(row[7]);
    const float* img = (const float*)t[0];
    const uint8_t* lbl = (const uint8_t*)t[1];
    const long Vs = (long)D * H * W;
    const int ra = d.ax0, rb = d.ax1, n = S[ra];
    double cnt[AUG_MAXC], sum[AUG_MAXC], sq[AUG_MAXC];
#pragma unroll
    for (int c = 0; c < AUG_MAXC; ++c) { cnt[c] = 0.0; sum[c] = 0.0; sq[c] = 0.0; }
    const bool warped = AFFINE && affine[(long)s * AUG_AROW] != 0.f;
    if (warped) {
        float m[9], half[3], centre[3];
#pragma unroll
        for (int j = 0; j < 9; ++j) m[j] = affine[(long)s * AUG_AROW + 7 + j];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            half[a] = (float)(S[a] - 1) * 0.5f;
            centre[a] = (float)c0[a] + half[a];
            ok = ok && dims[a] <= AUG_MAXDIM_AFFINE;
        }
        const int nb1 = (S[1] + AUG_BR1 - 1) / AUG_BR1, nb2 = (S[2] + AUG_BR2 - 1) / AUG_BR2;
        const int brick01 = blockIdx.x / nb2;
        int o[3];
        o[1] = (brick01 % nb1) * AUG_BR1 + (threadIdx.x >> 4);
        o[2] = (blockIdx.x % nb2) * AUG_BR2 + (threadIdx.x & 15);
#pragma unroll 2
        for (int i = 0; i < AUG_BR0; ++i) {
            o[0] = (brick01 / nb1) * AUG_BR0 + i;
            if (o[0] >= S[0] || o[1] >= S[1] || o[2] >= S[2]) continue;
            const long v = ((long)o[0] * S[1] + o[1]) * S[2] + o[2];
            int p[3];
            aug_crop_pos(o, S, k, ra, rb, n, flips, p);
            AugTaps tp;
            if (ok) tp = aug_affine_taps(p, m, half, centre, dims);
#pragma unroll
            for (int c = 0; c < AUG_MAXC; ++c) {
                if (c >= d.C) continue;
                float val = ok ? aug_trilinear(img + c * Vs, tp) : 0.f;
                if (shift) val = val + off;
                x[((long)s * d.C + c) * V + v] = val;
                if (NORM && val != 0.f) { cnt[c] += 1.0; sum[c] += (double)val; sq[c] += (double)val * (double)val; }
            }
#pragma unroll
            for (int l = 0; l < AUG_MAXC; ++l)
                if (l < d.L) y[((long)s * d.L + l) * V + v] = ok ? (float)lbl[l * Vs + tp.near] : 0.f;
        }
    } else
#pragma unroll
    for (int i = 0; i < AUG_VPT; ++i) {                      // unrolled: the loads of all AUG_VPT voxels are in flight together
        const long v = ((long)blockIdx.x * AUG_VPT + i) * 256 + threadIdx.x;
        if (v >= V) continue;
        int o[3];
        o[2] = (int)(v % S[2]);
        const long r = v / S[2];
        o[1] = (int)(r % S[1]);
        o[0] = (int)(r / S[1]);
        int p[3];
        aug_crop_pos(o, S, k, ra, rb, n, flips, p);
        const long src = ((long)(c0[0] + p[0]) * H + (c0[1] + p[1])) * W + (c0[2] + p[2]);
#pragma unroll
        for (int c = 0; c < AUG_MAXC; ++c) {
            if (c >= d.C) continue;
            float val = ok ? img[c * Vs + src] : 0.f;
            if (shift) val = val + off;
            x[((long)s * d.C + c) * V + v] = val;
            if (NORM && val != 0.f) { cnt[c] += 1.0; sum[c] += (double)val; sq[c] += (double)val * (double)val; }
        }
#pragma unroll
        for (int l = 0; l < AUG_MAXC; ++l)
            if (l < d.L) y[((long)s * d.L + l) * V + v] = ok ? (float)lbl[l * Vs + src] : 0.f;
    }
    if (NORM) {
        __shared__ double red[4][3];
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        for (int c = 0; c < d.C; ++c) {
            const double a = wave_sum_d(cnt[c]), b = wave_sum_d(sum[c]), e = wave_sum_d(sq[c]);
            if (lane == 0) { red[wv][0] = a; red[wv][1] = b; red[wv][2] = e; }
            __syncthreads();
            if (threadIdx.x < 3) {
                const int j = threadIdx.x;
                part[(((long)s * d.C + c) * gridDim.x + blockIdx.x) * 3 + j] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
            }
            __syncthreads();
        }
    }
}

// grid (AUG_NORM_WG, B * C): every workgroup reduces the nblk partials of its (sample, channel) in the same fixed order
__global__ void __launch_bounds__(256)
aug_norm_kernel(float* __restrict__ x, long V, const double* __restrict__ part, int nblk) {
    __shared__ double red[3][256];
    __shared__ float ms[2];
    const long bc = blockIdx.y;
    const double* pp = part + bc * nblk * 3;
    double a = 0.0, b = 0.0, e = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) { a += pp[i * 3]; b += pp[i * 3 + 1]; e += pp[i * 3 + 2]; }
    red[0][threadIdx.x] = a; red[1][threadIdx.x] = b; red[2][threadIdx.x] = e;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w)
            for (int j = 0; j < 3; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double cnt = red[0][0];
        const double mean = cnt > 0.0 ? red[1][0] / cnt : 0.0;
        const double var = cnt > 0.0 ? fmax(red[2][0] / cnt - mean * mean, 0.0) : 0.0;
        float sd = (float)sqrt(var);
        if (sd == 0.f) sd = 1.f;                              // NormalizeIntensity: std 0 -> 1
        ms[0] = (float)mean; ms[1] = sd;
    }
    __syncthreads();
    const float mean = ms[0], sd = ms[1];
    float* xp = x + bc * V;
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long)gridDim.x * 256) {
        const float val = xp[v];
        if (val != 0.f) xp[v] = (val - mean) / sd;           // no nonzero voxel: nothing to change
    }
}

bool aug_desc_ok(const UnetrAugDesc* d) {
    if (!d || d->B <= 0 || d->num_samples <= 0 || d->B % d->num_samples) return false;
    if (d->C <= 0 || d->C > AUG_MAXC || d->L <= 0 || d->L > AUG_MAXC) return false;
    const int S[3] = {d->S0, d->S1, d->S2};
    for (int a = 0; a < 3; ++a) if (S[a] <= 0 || S[a] > AUG_MAXS) return false;
    if (d->ax0 < 0 || d->ax0 > 2 || d->ax1 < 0 || d->ax1 > 2 || d->ax0 == d->ax1 || S[d->ax0] != S[d->ax1]) return false;
    if (d->max_k <= 0 || d->B > 65535) return false;
    return d->sampling == 0 || d->sampling == 1;
}

bool aug_affine_desc_ok(const UnetrAugAffineDesc* a) {
    if (!a || !(a->prob >= 0.0 && a->prob <= 1.0)) return false;
    for (int i = 0; i < 3; ++i) if (!(a->rotate[i] >= 0.0 && isfinite(a->rotate[i]))) return false;
    return a->zoom_lo > 0.0 && a->zoom_lo <= a->zoom_hi && isfinite(a->zoom_hi);
}

}  // namespace

extern "C" long unetr_aug_index_ws_ints(long V) { return V <= 0 ? 0 : 4L * cdiv(V, AUG_CHUNK) + 2; }

extern "C" int unetr_aug_prep(float* img, const float* lbl, int C, int L, int D, int H, int W, int scale_mode, float a_min,
                              float a_range, float b_range, float b_min, float b_max, int do_box, int* box, int* flag,
                              void* stream) {
    if (!img || !lbl || !box || !flag || C <= 0 || L <= 0 || D <= 0 || H <= 0 || W <= 0 || scale_mode < 0 || scale_mode > 2)
        return UNETR_ERR_ARG;
    const long V = (long)D * H * W;
    const int grid = (int)std::min<long>(cdiv(V, 256), 2048);
    hipLaunchKernelGGL(aug_prep_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, img, lbl, C, L, D, H, W, scale_mode,
                       a_min, a_range, b_range, b_min, b_max, do_box, box, flag);
    return hipGetLastError() == hipSuccess ? UNETR_OK : UNETR_ERR_LAUNCH;
}

extern "C" int unetr_aug_crop(const float* img, const float* lbl, int C, int L, int D, int H, int W, int z0, int y0, int x0,
                              int d, int h, int w, float* oimg, uint8_t* olbl, void* stream) {
    if (!img || !lbl || !oimg || !olbl || C <= 0 || L <= 0 || d <= 0 || h <= 0 || w <= 0 || z0 < 0 || y0 < 0 || x0 < 0 ||
        z0 + d > D || y0 + h > H || x0 + w > W || h > 65535 || (long)d * (C + L) > 65535)
        return UNETR_ERR_ARG;
    hipLaunchKernelGGL(aug_crop_kernel, dim3(cdiv(w, 256), h, d * (C + L)), dim3(256), 0, (hipStream_t)stream, img, lbl, C, L,
                       D, H, W, z0, y0, x0, d, h, w, oimg, olbl);
    return hipGetLastError() == hipSuccess ? UNETR_OK : UNETR_ERR_LAUNCH;
}

extern "C" int unetr_aug_index_count(const float* img, const uint8_t* lbl, int C, int L, long V, float thr, int* ws,
                                     size_t ws_ints, void* stream) {
    if (!img || !lbl || !ws || C <= 0 || L <= 0 || V <= 0 || V > 0x7fffffffL) return UNETR_ERR_ARG;
    if ((long)ws_ints < unetr_aug_index_ws_ints(V)) return UNETR_ERR_WORKSPACE;
    const int nblk = cdiv(V, AUG_CHUNK);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(aug_count_kernel, dim3(nblk), dim3(256), 0, st, img, lbl, C, L, V, thr, ws, nblk);
    hipLaunchKernelGGL(aug_scan_kernel, dim3(1), dim3(1024), 0, st, ws, nblk);
    return hipGetLastError() == hipSuccess ? UNETR_OK : UNETR_ERR_LAUNCH;
}

extern "C" int unetr_aug_index_scatter(const float* img, const uint8_t* lbl, int C, int L, long V, float thr, const int* ws,
                                       size_t ws_ints, int* fg, int* bg, void* stream) {
    if (!img || !lbl || !ws || !fg || !bg || C <= 0 || L <= 0 || V <= 0 || V > 0x7fffffffL) return UNETR_ERR_ARG;
    if ((long)ws_ints < unetr_aug_index_ws_ints(V)) return UNETR_ERR_WORKSPACE;
    const int nblk = cdiv(V, AUG_CHUNK);
    hipLaunchKernelGGL(aug_scatter_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, img, lbl, C, L, V, thr, ws, nblk,
                       fg, bg);
    return hipGetLastError() == hipSuccess ? UNETR_OK : UNETR_ERR_LAUNCH;
}

extern "C" int unetr_aug_sample(const UnetrAugDesc* d, const long long* vols, int nvol, const int* order, long long* state,
                                int* params, void* stream) {
    if (!aug_desc_ok(d) || !vols || nvol <= 0 || !order || !state || !params) return UNETR_ERR_ARG;
    hipLaunchKernelGGL(aug_sample_kernel<false>, dim3(1), dim3(256), 0, (hipStream_t)stream, *d, UnetrAugAffineDesc{}, vols, nvol,
                       order, state, params, (float*)nullptr);
    return hipGetLastError() == hipSuccess ? UNETR_OK : UNETR_ERR_LAUNCH;
}

extern "C" int unetr_aug_sample_affine(const UnetrAugDesc* d, const UnetrAugAffineDesc* a, const long long* vols, int nvol,
                                       const int* order, long long* state, int* params, float* affine, void* stream) {
    if (!aug_desc_ok(d) || !aug_affine_desc_ok(a) || !vols || nvol <= 0 || !order || !state || !params || !affine)
        return UNETR_ERR_ARG;
    hipLaunchKernelGGL(aug_sample_kernel<true>, dim3(1), dim3(256), 0, (hipStream_t)stream, *d, *a, vols, nvol, order, state,
                       params, affine);
    return hipGetLastError() == hipSuccess ? UNETR_OK : UNETR_ERR_LAUNCH;
}

extern "C" size_t unetr_aug_gather_ws_bytes(const UnetrAugDesc* d) {
    if (!aug_desc_ok(d) || !d->normalize) return 0;
    const long V = (long)d->S0 * d->S1 * d->S2;
    return (size_t)d->B * d->C * cdiv(V, AUG_TILE) * 3 * sizeof(double);
}

extern "C" int unetr_aug_gather(const UnetrAugDesc* d, const long long* vols, int nvol, const int* params, float* x, float* y,
                                void* ws, size_t ws_bytes, void* stream) {
    if (!aug_desc_ok(d) || !vols || nvol <= 0 || !params || !x || !y) return UNETR_ERR_ARG;
    if (d->normalize && (!ws || ws_bytes < unetr_aug_gather_ws_bytes(d))) return UNETR_ERR_WORKSPACE;
    const long V = (long)d->S0 * d->S1 * d->S2;
    const int nblk = cdiv(V, AUG_TILE);
    hipStream_t st = (hipStream_t)stream;
    if (d->normalize) {
        hipLaunchKernelGGL((aug_gather_kernel<true, false>), dim3(nblk, d->B), dim3(256), 0, st, *d, vols, nvol, params,
                           (const float*)nullptr, x, y, (double*)ws);
        hipLaunchKernelGGL(aug_norm_kernel, dim3(AUG_NORM_WG, d->B * d->C), dim3(256), 0, st, x, V, (const double*)ws, nblk);
    } else {
        hipLaunchKernelGGL((aug_gather_kernel<false, false>), dim3(nblk, d->B), dim3(256), 0, st, *d, vols, nvol, params,
                           (const float*)nullptr, x, y, (double*)nullptr);
    }
    return hipGetLastError() == hipSuccess ? UNETR_OK : UNETR_ERR_LAUNCH;
}

extern "C" size_t unetr_aug_gather_affine_ws_bytes(const UnetrAugDesc* d) {
    if (!aug_desc_ok(d) || !d->normalize) return 0;
    return (size_t)d->B * d->C * aug_affine_blocks(d) * 3 * sizeof(double);
}

extern "C" int unetr_aug_gather_affine(const UnetrAugDesc* d, const long long* vols, int nvol, const int* params,
                                       const float* affine, float* x, float* y, void* ws, size_t ws_bytes, void* stream) {
    if (!aug_desc_ok(d) || !vols || nvol <= 0 || !params || !affine || !x || !y) return UNETR_ERR_ARG;
    if (d->normalize && (!ws || ws_bytes < unetr_aug_gather_affine_ws_bytes(d))) return UNETR_ERR_WORKSPACE;
    const long V = (long)d->S0 * d->S1 * d->S2;
    const int nblk = aug_affine_blocks(d);
    hipStream_t st = (hipStream_t)stream;
    if (d->normalize) {
        hipLaunchKernelGGL((aug_gather_kernel<true, true>), dim3(nblk, d->B), dim3(256), 0, st, *d, vols, nvol, params, affine, x,
                           y, (double*)ws);
        hipLaunchKernelGGL(aug_norm_kernel, dim3(AUG_NORM_WG, d->B * d->C), dim3(256), 0, st, x, V, (const double*)ws, nblk);
    } else {
        hipLaunchKernelGGL((aug_gather_kernel<false, true>), dim3(nblk, d->B), dim3(256), 0, st, *d, vols, nvol, params, affine, x,
                           y, (double*)nullptr);
    }
    return hipGetLastError() == hipSuccess ? UNETR_OK : UNETR_ERR_LAUNCH;
}
