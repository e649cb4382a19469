// GPU-resident random crop sampling and augmentation: the per-step random part of the reference's
// training transforms (unetr_segmentation_3d.py:322-476, unetr_ranking_pretraining_3d.py:346-444), MONAI 0.6.0 semantics as
// restated in tests/augment_ref.py.
//
// VolumeCache.add (setup, may synchronise):
//   aug_prep_kernel      ScaleIntensityRanged (same float32 operations as MONAI, no contraction) in place, the bounding box
//                        of any_c(image > 0) by integer atomics, a flag for label values that are not integers in 0..255
//   aug_crop_kernel      copies the foreground box: image float32, label uint8
//   aug_count_kernel<2>    per chunk of AUG_CHUNK voxels the number of foreground / background voxels of map_binary_to_indices
//   aug_scan_kernel        one workgroup per list: exclusive scan of its chunk counts and the list's length
//   aug_scatter_kernel<2>  ordered compaction: each chunk again, AUG_CHUNK / 256 rounds of ballot + prefix, ascending ravel order
// VolumeCache.build_class_indices (setup, may synchronise): map_classes_to_indices, the same three kernels (<0>) for K <= 32 lists
// at once: one ballot per class from one read of the label, a stable counting sort; between scan and scatter
//   aug_class_offsets_kernel   where each list starts in the concatenated array (int64)
// RandCropAugment.__call__ (per step: launches only, no host sync, no allocation):
//   aug_sample_kernel    one workgroup: Philox4x64-10 draws, crop centres, the params table, counter and cursor advance;
//                        <true, .> also draws the rotation / zoom of each sample and writes the affine table; <., true> takes
//                        the crop centre from the list of a class drawn by the device ratios (RandCropByLabelClassesd)
//   aug_gather_kernel    every output voxel back through rot90^k, the flips and the corner to its source voxel; C image
//                        channels (+ shift) and L label bytes; with normalize also fp64 partial sums per workgroup;
//                        <., true> takes the samples its affine table flags through the matrix to a position between
//                        voxels of the whole volume: trilinear image, nearest label, border padding (aug_affine_voxel)
//   aug_norm_kernel      fixed-order reduction of the partials and (x - mean) / std over the nonzero voxels
// with an IntensityAugment (this project's own semantics), per call five more launches on x alone:
//   aug_intensity_sample_kernel   one workgroup, before aug_sample_kernel: Philox blocks 5..7, the intensity table
//   aug_blur_strided_kernel x 2, aug_blur_rows_kernel   separable Gaussian blur: axis 0 x -> ws, axis 1 ws -> x, axis 2 in place
//   aug_intensity_point_kernel    counter-based Gaussian noise, brightness, (min, max, fp64 sum) partials per channel
//   aug_intensity_tone_kernel     contrast and gamma from those statistics
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
constexpr int AUG_MAXK = 32;          // classes of the per-class voxel lists (one bit each)
constexpr int AUG_CCOLS = 2;          // int64 per class table row: concatenated lists (int32) ptr, offsets (int64 [K + 1]) ptr
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

// ---------------------------------------------------------------- add() / build_class_indices(): one ordered compaction
// map_binary_to_indices (the foreground and the background list) and map_classes_to_indices (K <= AUG_MAXK class lists) are the same
// stable counting sort with another membership rule: bit c of a voxel's word says that it is in list c.
// fg / bg: bit 0 = any label channel nonzero, bit 1 = not that and any image channel > thr.
__device__ __forceinline__ unsigned fg_bg(const float* __restrict__ img, const uint8_t* __restrict__ lbl, int C, int L, long V,
                                          float thr, long v) {
    bool fg = false;
#pragma clang loop vectorize(disable)                        // (the stride is V: a vector body would only serve V == 1)
    for (int l = 0; l < L; ++l) fg |= lbl[(long)l * V + v] != 0;
    bool any = false;
#pragma clang loop vectorize(disable)
    for (int c = 0; c < C; ++c) any |= img[(long)c * V + v] > thr;
    return (unsigned)fg | (unsigned)(!fg && any) << 1;
}

// classes.  L == 1: class ids, an id >= K is in no list; L > 1 (K == L): channel c is nonzero, lists may overlap.  masked: no list
// takes a voxel outside any_c(img > thr).
__device__ __forceinline__ unsigned class_bits(const float* __restrict__ img, const uint8_t* __restrict__ lbl, int C, int L, int K,
                                               long V, int masked, float thr, long v) {
    unsigned bits = 0u;
    if (L == 1) {
        const int id = lbl[v];
        if (id < K) bits = 1u << id;
    } else {
        for (int l = 0; l < L; ++l) bits |= (unsigned)(lbl[(long)l * V + v] != 0) << l;
    }
    if (masked && bits) {
        bool any = false;
        for (int c = 0; c < C; ++c) any |= img[(long)c * V + v] > thr;
        if (!any) bits = 0u;
    }
    return bits;
}

// KT = 2: the fg / bg pair, two lists known at compile time; KT = 0: K class lists, K at run time
struct AugMember { const float* img; const uint8_t* lbl; int C, L, K; long V; int masked; float thr; };
template <int KT>
__device__ __forceinline__ unsigned aug_list_bits(const AugMember& m, long v) {
    if (v >= m.V) return 0u;
    return KT ? fg_bg(m.img, m.lbl, m.C, m.L, m.V, m.thr, v) : class_bits(m.img, m.lbl, m.C, m.L, m.K, m.V, m.masked, m.thr, v);
}

// ws (ints): [cnt K][nblk][off K][nblk], list-major (fg / bg: + its two totals).  Per chunk of AUG_CHUNK voxels the number of voxels
// of every list, from one read of the volume: lane c of every wave keeps the count of list c, one ballot per list and round, no atomics.
template <int KT>
__global__ void __launch_bounds__(256) aug_count_kernel(AugMember m, int* __restrict__ ws, int nblk) {
    const int K = KT ? KT : m.K;
    __shared__ int red[4][AUG_MAXK];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int mine = 0;
    const long base = (long)blockIdx.x * AUG_CHUNK;
    for (int i = 0; i < AUG_CHUNK / 256; ++i) {
        const unsigned bits = aug_list_bits<KT>(m, base + i * 256 + threadIdx.x);
        for (int c = 0; c < K; ++c) {
            const int n = __popcll(__ballot(bits >> c & 1u));
            if (lane == c) mine += n;
        }
    }
    if (lane < K) red[wv][lane] = mine;
    __syncthreads();
    if (threadIdx.x < K)
        ws[(long)threadIdx.x * nblk + blockIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// one workgroup of 1024 threads per list: exclusive scan of its chunk counts -- thread t scans a contiguous segment, thread 0 the
// 1024 segment sums -- and the list's length to totals[list] (fg / bg: the two ints behind ws; classes: offsets[1..K], int64)
template <typename T>
__global__ void __launch_bounds__(1024) aug_scan_kernel(int* __restrict__ ws, int nblk, T* __restrict__ totals) {
    __shared__ int seg[1024];
    const int per = (nblk + 1023) / 1024;
    const int b0 = min(nblk, (int)threadIdx.x * per), b1 = min(nblk, b0 + per);
    const int* cnt = ws + (long)blockIdx.x * nblk;
    int* off = ws + ((long)gridDim.x + blockIdx.x) * nblk;
    int s = 0;
    for (int b = b0; b < b1; ++b) s += cnt[b];
    seg[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < 1024; ++t) { const int v = seg[t]; seg[t] = run; run += v; }
        totals[blockIdx.x] = run;
    }
    __syncthreads();
    int run = seg[threadIdx.x];
    for (int b = b0; b < b1; ++b) { off[b] = run; run += cnt[b]; }
}

// offsets [K + 1] (int64) from the K list lengths the scan left in offsets[1..K]: where each list starts in the concatenated
// array, in class order; offsets[K] is the total
__global__ void aug_class_offsets_kernel(long long* __restrict__ offsets, int K) {
    if (threadIdx.x == 0) {
        long long run = 0;
        offsets[0] = 0;
        for (int c = 1; c <= K; ++c) { run += offsets[c]; offsets[c] = run; }
    }
}

// The slot of a voxel in its list: where the list starts (fg / bg: l0 and l1; classes: l0 + offsets[c]), the scanned offset of the
// chunk plus what earlier rounds of the chunk put there (run), the waves before this one in the round (wtot) and the lanes below in
// the wave (ballot).  Every term counts voxels at lower ravel indices, so each list is ascending and the same on every run.
// run and wtot alternate between two copies, so a round needs one barrier: what round i writes was last read in round i - 1.
template <int KT>
__global__ void __launch_bounds__(256)
aug_scatter_kernel(AugMember m, const int* __restrict__ ws, int nblk, int* __restrict__ l0, int* __restrict__ l1,
                   const long long* __restrict__ offsets) {
    const int K = KT ? KT : m.K;
    __shared__ int wtot[2][AUG_MAXK][4];
    __shared__ int run[2][AUG_MAXK];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    if (threadIdx.x < K) run[0][threadIdx.x] = ws[((long)K + threadIdx.x) * nblk + blockIdx.x];
    const long base = (long)blockIdx.x * AUG_CHUNK;
    for (int i = 0; i < AUG_CHUNK / 256; ++i) {
        const int q = i & 1;
        const long v = base + i * 256 + threadIdx.x;
        const unsigned bits = aug_list_bits<KT>(m, v);
        for (int c = 0; c < K; ++c) {
            const int n = __popcll(__ballot(bits >> c & 1u));
            if (lane == 0) wtot[q][c][wv] = n;
        }
        __syncthreads();
        if (threadIdx.x < K)
            run[q ^ 1][threadIdx.x] = run[q][threadIdx.x] + wtot[q][threadIdx.x][0] + wtot[q][threadIdx.x][1] + wtot[q][threadIdx.x][2] +
                                      wtot[q][threadIdx.x][3];
        for (int c = 0; c < K; ++c) {
            const unsigned long long mk = __ballot(bits >> c & 1u);
            if (!mk) continue;                               // (wave-uniform) no voxel of list c in this wave's 64
            int p = run[q][c] + __popcll(mk & below);
            for (int k = 0; k < wv; ++k) p += wtot[q][c][k];
            int* list = KT ? (c ? l1 : l0) : l0 + offsets[c];
            if (bits >> c & 1u) list[p] = (int)v;
        }
    }
}

// ---------------------------------------------------------------- per call: sampler
// state (int64): [call counter, cursor, len(order), 0]
// AFFINE: block 3 word 0 flags the sample, words 1..3 are the angles about axes 0..2, block 4 words 0..2 the zooms (word 0
// for all three unless zoom_per_axis); blocks 0..2 are drawn as without it.  Angles and zooms are lo + (hi - lo) * u in
// double, stored as float32; M = (R0 . R1) . R2 . diag(1 / z) in double from the STORED values, rounded once.
// CLASSES (RandCropByLabelClassesd, d.sampling == 2): block 0 word 0 picks the class by the DEVICE ratios, word 1 the voxel of
// that class; every other word is drawn as without it.  affine may be null there: no block 3 / 4 draws, no affine table.
struct AugClassArgs {
    const long long* table;           // [nvol][AUG_CCOLS]
    const float* ratios;              // [K], read on every call
    int* classes;                     // [B]: the class drawn, -1 on the uniform fallback
    int K;
};

// generate_label_classes_crop_centers for one sample: a class absent from the volume, or whose ratio is not a positive finite
// number, has weight 0; the class is the first c with u * total < cum_c (sums in class order, double), the last weighted class
// if rounding falls through; -1 when no class has weight, and the caller takes the uniform corner.  Never names an empty list.
__device__ __forceinline__ int aug_pick_class(const float* __restrict__ ratios, const long long* __restrict__ offs, int K, double u) {
#pragma clang fp contract(off)
    double total = 0.0;
    int last = -1;
    for (int c = 0; c < K; ++c) {
        const float r = ratios[c];
        const double e = offs[c + 1] > offs[c] && r > 0.f && isfinite(r) ? (double)r : 0.0;
        total += e;
        if (e > 0.0) last = c;
    }
    if (last < 0) return -1;
    const double t = u * total;
    double cum = 0.0;
    for (int c = 0; c < K; ++c) {
        const float r = ratios[c];
        const double e = offs[c + 1] > offs[c] && r > 0.f && isfinite(r) ? (double)r : 0.0;
        cum += e;
        if (e > 0.0 && t < cum) return c;
    }
    return last;
}

template <bool AFFINE, bool CLASSES>
__global__ void __launch_bounds__(256)
aug_sample_kernel(UnetrAugDesc d, UnetrAugAffineDesc af, const long long* __restrict__ vols, int nvol,
                  const int* __restrict__ order, long long* __restrict__ state, int* __restrict__ params,
                  float* __restrict__ affine, AugClassArgs cl) {
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
        long long idx = -1;                                  // the centre voxel; -1: draw the corner uniformly
        if (CLASSES) {                                       // RandCropByLabelClassesd
            const long long* ct = cl.table + (long)vol * AUG_CCOLS;
            const long long* offs = (const long long*)ct[1];
            const int cls = aug_pick_class(cl.ratios, offs, cl.K, u01(w0.v[0]));
            if (cls >= 0)
                idx = ((const int*)ct[0])[offs[cls] + randint(w0.v[1], (unsigned long long)(offs[cls + 1] - offs[cls]))];
            cl.classes[s] = cls;
        } else if (d.sampling == 0) {                        // RandCropByPosNegLabeld
            const long long nfg = t[3], nbg = t[5];
            const double pr = nfg == 0 ? 0.0 : (nbg == 0 ? 1.0 : d.pos_ratio);
            const bool pos = u01(w0.v[0]) < pr;
            const long long len = pos ? nfg : nbg;
            const int* list = (const int*)(pos ? t[2] : t[4]);
            idx = list[randint(w0.v[1], (unsigned long long)len)];
        }
        if (idx >= 0) {
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

// ---------------------------------------------------------------- per call: intensity augmentation (this project's semantics)
// table (int32 [B][AUG_IROW], floats as their bits): flag bits (noise 1, blur 2, brightness 4, contrast 8, gamma 16), noise std,
// blur sigma of axis 0, 1, 2, brightness factor, contrast factor, gamma, low / high word of the call counter n, six zeros.
// Everything below runs on x only, after the gather (+ normalize): blur, noise, brightness, contrast, gamma.  float32, no
// contraction, in the one order tests/augment_intensity_ref.py restates.  Flags are read from the table, so the workgroups of a
// sample whose flag is clear return at once, uniformly; grids are fixed.
constexpr int AUG_IROW = 16;
constexpr int AUG_I_NOISE = 1, AUG_I_BLUR = 2, AUG_I_BRIGHT = 4, AUG_I_CONTRAST = 8, AUG_I_GAMMA = 16;
constexpr int AUG_BLUR_MAXR = 8;      // R = (int)(max(4 sigma, 0.5) + 0.5) with sigma <= 2
constexpr int AUG_BLUR_T = 16;        // outputs per thread along a strided axis
constexpr int AUG_BLUR_LDS = 2048;    // floats of whole rows one workgroup stages for the pass along axis 2 (>= AUG_MAXS)
constexpr int AUG_TONE_TILE = 4096;   // voxels per workgroup of the contrast / gamma pass (a multiple of 1024)
constexpr int AUG_NOISE_BLOCK = 16;  // Philox block of channel 0's noise: counter (n, s, 16 + c, 1 + group of 8 voxels)
static_assert(AUG_BLUR_LDS >= AUG_MAXS, "one row fits");

// blocks 5..7 of the sample's stream; blocks 0..4 are aug_sample_kernel's and do not move.  Reads state[0], writes no state.
__global__ void __launch_bounds__(256)
aug_intensity_sample_kernel(UnetrAugDesc d, UnetrAugIntensityDesc it, const long long* __restrict__ state, int* __restrict__ table) {
#pragma clang fp contract(off)
    const unsigned long long n = (unsigned long long)state[0];
    for (int s = threadIdx.x; s < d.B; s += 256) {
        const Ph4 w5 = aug_block(d.seed, n, s, 5), w6 = aug_block(d.seed, n, s, 6), w7 = aug_block(d.seed, n, s, 7);
        const unsigned long long fw[5] = {w5.v[0], w5.v[2], w5.v[3], w7.v[0], w7.v[2]};      // flag word of noise, blur, brightness, contrast, gamma
        const unsigned long long vw[5] = {w5.v[1], 0ull, w6.v[3], w7.v[1], w7.v[3]};          // value word (the blur has three, below)
        int flags = 0;
        float val[5] = {0.f, 0.f, 1.f, 1.f, 1.f}, sg[3] = {0.f, 0.f, 0.f};
        for (int j = 0; j < 5; ++j) {
            if (!(u01(fw[j]) < it.prob[j])) continue;
            flags |= 1 << j;
            if (j == 1) for (int a = 0; a < 3; ++a) sg[a] = (float)(it.lo[1] + (it.hi[1] - it.lo[1]) * u01(w6.v[a]));
            else val[j] = (float)(it.lo[j] + (it.hi[j] - it.lo[j]) * u01(vw[j]));
        }
        int* row = table + (long)s * AUG_IROW;
        row[0] = flags; row[1] = __float_as_int(val[0]);
        for (int a = 0; a < 3; ++a) row[2 + a] = __float_as_int(sg[a]);
        row[5] = __float_as_int(val[2]); row[6] = __float_as_int(val[3]); row[7] = __float_as_int(val[4]);
        row[8] = (int)(unsigned)(n & 0xffffffffull); row[9] = (int)(unsigned)(n >> 32);
        for (int j = 10; j < AUG_IROW; ++j) row[j] = 0;
    }
}

// normalised taps w[0 .. 2R] of one axis into LDS (g, w: 2 * AUG_BLUR_MAXR + 1 floats each); every thread of the workgroup calls
// it.  g_k = expf(-(float)(k k) / (2 sigma sigma)), w_k = g_k / sum(g), the sum in order k = -R .. R.  A sigma that is not
// positive (possible only in a device table nobody checked) gives the single tap 1.
__device__ __forceinline__ int aug_blur_weights(float sigma, float* g, float* w) {
#pragma clang fp contract(off)
    int R = 0;
    if (sigma > 0.f) R = (int)fminf(fmaxf(4.0f * sigma, 0.5f) + 0.5f, (float)AUG_BLUR_MAXR);
    const int t = threadIdx.x;
    if (t <= 2 * R) {
        const int k = t - R;
        g[t] = R ? expf(-(float)(k * k) / (2.0f * sigma * sigma)) : 1.f;
    }
    __syncthreads();
    if (t <= 2 * R) {
        float sum = 0.f;
        for (int j = 0; j <= 2 * R; ++j) sum = sum + g[j];
        w[t] = g[t] / sum;
    }
    __syncthreads();
    return R;
}

// AUG_BLUR_T outputs a0 .. of one column: the window of AUG_BLUR_T + 2R inputs (indices clamped into the crop: border padding)
// sits in registers, every index a compile-time constant
template <int R>
__device__ __forceinline__ void aug_blur_column(const float* __restrict__ src, float* __restrict__ dst, long base, long stride,
                                                int A, int a0, const float* w) {
#pragma clang fp contract(off)
    float win[AUG_BLUR_T + 2 * R], wk[2 * R + 1];
#pragma unroll
    for (int j = 0; j < AUG_BLUR_T + 2 * R; ++j) win[j] = src[base + (long)min(max(a0 + j - R, 0), A - 1) * stride];
#pragma unroll
    for (int k = 0; k <= 2 * R; ++k) wk[k] = w[k];
#pragma unroll
    for (int i = 0; i < AUG_BLUR_T; ++i) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k <= 2 * R; ++k) acc = acc + wk[k] * win[i + k];
        if (a0 + i < A) dst[base + (long)(a0 + i) * stride] = acc;
    }
}

// the pass along axis 0 or 1: a sample's [C][S0][S1][S2] block seen as [outer][A][inner], one thread per (outer, inner) column,
// neighbouring threads on neighbouring inner positions (coalesced as they stand).  grid (ceil(outer inner / 256), ceil(A / T), B)
__global__ void __launch_bounds__(256)
aug_blur_strided_kernel(const int* __restrict__ table, int axis, const float* __restrict__ src, float* __restrict__ dst, long sample_elems,
                        long outer, int A, long inner) {
    __shared__ float g[2 * AUG_BLUR_MAXR + 1], w[2 * AUG_BLUR_MAXR + 1];
    const int s = blockIdx.z;
    const int* row = table + (long)s * AUG_IROW;
    if (!(row[0] & AUG_I_BLUR)) return;
    const int R = aug_blur_weights(__int_as_float(row[2 + axis]), g, w);
    const long col = (long)blockIdx.x * 256 + threadIdx.x;
    if (col >= outer * inner) return;
    const long base = (long)s * sample_elems + (col / inner) * A * inner + col % inner;
    const int a0 = blockIdx.y * AUG_BLUR_T;
    switch (R) {
        case 0: aug_blur_column<0>(src, dst, base, inner, A, a0, w); break;
        case 1: aug_blur_column<1>(src, dst, base, inner, A, a0, w); break;
        case 2: aug_blur_column<2>(src, dst, base, inner, A, a0, w); break;
        case 3: aug_blur_column<3>(src, dst, base, inner, A, a0, w); break;
        case 4: aug_blur_column<4>(src, dst, base, inner, A, a0, w); break;
        case 5: aug_blur_column<5>(src, dst, base, inner, A, a0, w); break;
        case 6: aug_blur_column<6>(src, dst, base, inner, A, a0, w); break;
        case 7: aug_blur_column<7>(src, dst, base, inner, A, a0, w); break;
        default: aug_blur_column<8>(src, dst, base, inner, A, a0, w); break;
    }
}

// the pass along axis 2: a workgroup stages nr whole rows (nr S2 <= AUG_BLUR_LDS contiguous floats) in LDS and writes them
// back blurred, so src may be dst.  grid (ceil(rows / nr), B), rows = C S0 S1
__global__ void __launch_bounds__(256)
aug_blur_rows_kernel(const int* __restrict__ table, const float* src, float* dst, long rows, int S2, int nr) {
#pragma clang fp contract(off)
    __shared__ float g[2 * AUG_BLUR_MAXR + 1], w[2 * AUG_BLUR_MAXR + 1];
    __shared__ float buf[AUG_BLUR_LDS];
    const int s = blockIdx.y;
    const int* row = table + (long)s * AUG_IROW;
    if (!(row[0] & AUG_I_BLUR)) return;
    const int R = aug_blur_weights(__int_as_float(row[4]), g, w);
    const long r0 = (long)blockIdx.x * nr;
    const int cnt = (int)(rows - r0 < nr ? rows - r0 : nr) * S2;
    const long base = ((long)s * rows + r0) * S2;
    for (int e = threadIdx.x; e < cnt; e += 256) buf[e] = src[base + e];
    __syncthreads();
    for (int e = threadIdx.x; e < cnt; e += 256) {
        const int r = e / S2, i = e - r * S2;
        float acc = 0.f;
        for (int k = -R; k <= R; ++k) acc = acc + w[k + R] * buf[r * S2 + min(max(i + k, 0), S2 - 1)];
        dst[base + e] = acc;
    }
}

// noise and brightness in place, and the (min, max, fp64 sum) of what they leave, per workgroup, for contrast and gamma.
// One thread per group of 8 consecutive voxels of a channel: one Philox block, four Box-Muller pairs.
// grid (ceil(V / AUG_TILE), C, B); part_sum / part_min / part_max: [B][C][gridDim.x]
__global__ void __launch_bounds__(256)
aug_intensity_point_kernel(UnetrAugDesc d, const int* __restrict__ table, float* __restrict__ x, double* __restrict__ part_sum,
                           float* __restrict__ part_min, float* __restrict__ part_max) {
#pragma clang fp contract(off)
    const int s = blockIdx.z, c = blockIdx.y;
    const int* row = table + (long)s * AUG_IROW;
    const int flags = row[0];
    if (!(flags & (AUG_I_NOISE | AUG_I_BRIGHT | AUG_I_CONTRAST | AUG_I_GAMMA))) return;
    const long V = (long)d.S0 * d.S1 * d.S2;
    const long grp = (long)blockIdx.x * 256 + threadIdx.x;
    const long v0 = grp * AUG_VPT;
    const int cnt = V - v0 >= AUG_VPT ? AUG_VPT : (V > v0 ? (int)(V - v0) : 0);
    float* xp = x + ((long)s * d.C + c) * V + v0;
    const bool vec = cnt == AUG_VPT && ((size_t)xp & 15) == 0;
    float val[AUG_VPT];
    if (vec) {
        const float4 lo = ((const float4*)xp)[0], hi = ((const float4*)xp)[1];
        val[0] = lo.x; val[1] = lo.y; val[2] = lo.z; val[3] = lo.w; val[4] = hi.x; val[5] = hi.y; val[6] = hi.z; val[7] = hi.w;
    } else {
#pragma unroll
        for (int j = 0; j < AUG_VPT; ++j) val[j] = j < cnt ? xp[j] : 0.f;
    }
    if ((flags & AUG_I_NOISE) && cnt > 0) {
        const float sd = __int_as_float(row[1]);
        Ph4 ctr;
        ctr.v[0] = (unsigned long long)(unsigned)row[8] | (unsigned long long)(unsigned)row[9] << 32;
        ctr.v[1] = (unsigned long long)s; ctr.v[2] = (unsigned long long)(AUG_NOISE_BLOCK + c); ctr.v[3] = 1ull + (unsigned long long)grp;
        const Ph4 r4 = philox4x64(ctr, d.seed, 0ull);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned a = (unsigned)(r4.v[i] & 0xffffffffull), b = (unsigned)(r4.v[i] >> 32);
            const float u1 = ((float)(a >> 8) + 0.5f) * 0x1p-24f, u2 = ((float)(b >> 8) + 0.5f) * 0x1p-24f;
            const float r = sqrtf(-2.0f * logf(u1)), t = 6.283185307179586f * u2;
            val[2 * i] = val[2 * i] + sd * (r * cosf(t));
            val[2 * i + 1] = val[2 * i + 1] + sd * (r * sinf(t));
        }
    }
    if (flags & AUG_I_BRIGHT) {
        const float f = __int_as_float(row[5]);
#pragma unroll
        for (int j = 0; j < AUG_VPT; ++j) val[j] = val[j] * f;
    }
    if (flags & (AUG_I_NOISE | AUG_I_BRIGHT)) {
        if (vec) {
            ((float4*)xp)[0] = make_float4(val[0], val[1], val[2], val[3]);
            ((float4*)xp)[1] = make_float4(val[4], val[5], val[6], val[7]);
        } else {
#pragma unroll
            for (int j = 0; j < AUG_VPT; ++j) if (j < cnt) xp[j] = val[j];
        }
    }
    if (flags & (AUG_I_CONTRAST | AUG_I_GAMMA)) {
        __shared__ double rs[4];
        __shared__ float rmn[4], rmx[4];
        double sum = 0.0;
        float mn = INFINITY, mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < AUG_VPT; ++j)
            if (j < cnt) { sum += (double)val[j]; mn = fminf(mn, val[j]); mx = fmaxf(mx, val[j]); }
        sum = wave_sum_d(sum);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o, 64)); mx = fmaxf(mx, __shfl_xor(mx, o, 64)); }
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        if (lane == 0) { rs[wv] = sum; rmn[wv] = mn; rmx[wv] = mx; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const long p = ((long)s * d.C + c) * gridDim.x + blockIdx.x;
            part_sum[p] = ((rs[0] + rs[1]) + rs[2]) + rs[3];
            part_min[p] = fminf(fminf(rmn[0], rmn[1]), fminf(rmn[2], rmn[3]));
            part_max[p] = fmaxf(fmaxf(rmx[0], rmx[1]), fmaxf(rmx[2], rmx[3]));
        }
    }
}

// contrast about the channel mean, clamped to the channel's range, then gamma on the range contrast leaves: contrast is a
// monotone map and a clamp, so that range is the map of (mn, mx) and needs no second reduction.  Every workgroup of a
// (sample, channel) reduces the nblk partials in the same fixed order, then takes one tile of AUG_TONE_TILE voxels (the
// normalize pass's 64 looping workgroups per channel are too few waves to hide powf behind the loads: DESIGN.md section 12).
// grid (ceil(V / AUG_TONE_TILE), C, B)
__device__ __forceinline__ float aug_contrast(float v, float mean, float f, float mn, float mx) {
#pragma clang fp contract(off)
    return fminf(fmaxf((v - mean) * f + mean, mn), mx);
}

__global__ void __launch_bounds__(256)
aug_intensity_tone_kernel(UnetrAugDesc d, const int* __restrict__ table, float* __restrict__ x, const double* __restrict__ part_sum,
                          const float* __restrict__ part_min, const float* __restrict__ part_max, int nblk) {
#pragma clang fp contract(off)
    __shared__ double rs[256];
    __shared__ float rmn[256], rmx[256];
    const int s = blockIdx.z, c = blockIdx.y;
    const int* row = table + (long)s * AUG_IROW;
    const int flags = row[0];
    if (!(flags & (AUG_I_CONTRAST | AUG_I_GAMMA))) return;
    const long V = (long)d.S0 * d.S1 * d.S2;
    const long p0 = ((long)s * d.C + c) * nblk;
    double sum = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = threadIdx.x; i < nblk; i += 256) {
        sum += part_sum[p0 + i]; mn = fminf(mn, part_min[p0 + i]); mx = fmaxf(mx, part_max[p0 + i]);
    }
    rs[threadIdx.x] = sum; rmn[threadIdx.x] = mn; rmx[threadIdx.x] = mx;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            rs[threadIdx.x] += rs[threadIdx.x + w];
            rmn[threadIdx.x] = fminf(rmn[threadIdx.x], rmn[threadIdx.x + w]);
            rmx[threadIdx.x] = fmaxf(rmx[threadIdx.x], rmx[threadIdx.x + w]);
        }
        __syncthreads();
    }
    const float mean = (float)(rs[0] / (double)V);
    mn = rmn[0]; mx = rmx[0];
    const bool contrast = flags & AUG_I_CONTRAST, gam = flags & AUG_I_GAMMA;
    const float f = __int_as_float(row[6]), gamma = __int_as_float(row[7]);
    const float gmn = contrast ? aug_contrast(mn, mean, f, mn, mx) : mn, gmx = contrast ? aug_contrast(mx, mean, f, mn, mx) : mx;
    const float rng = gmx - gmn, den = rng + 1e-7f;
    float* xp = x + ((long)s * d.C + c) * V;
    const bool aligned = ((size_t)xp & 15) == 0;
    const long tile0 = (long)blockIdx.x * AUG_TONE_TILE;
#pragma unroll
    for (int i = 0; i < AUG_TONE_TILE / 1024; ++i) {          // 16 bytes per thread and round where the address allows
        const long v = tile0 + ((long)i * 256 + threadIdx.x) * 4;
        if (v >= V) continue;
        float q[4];
        const int cnt = V - v >= 4 ? 4 : (int)(V - v);
        const bool vec = aligned && cnt == 4;
        if (vec) { const float4 t = *(const float4*)(xp + v); q[0] = t.x; q[1] = t.y; q[2] = t.z; q[3] = t.w; }
        else
#pragma unroll
            for (int j = 0; j < 4; ++j) q[j] = j < cnt ? xp[v + j] : 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (contrast) q[j] = aug_contrast(q[j], mean, f, mn, mx);
            if (gam) q[j] = powf((q[j] - gmn) / den, gamma) * rng + gmn;
        }
        if (vec) *(float4*)(xp + v) = make_float4(q[0], q[1], q[2], q[3]);
        else
#pragma unroll
            for (int j = 0; j < 4; ++j) if (j < cnt) xp[v + j] = q[j];
    }
}

bool aug_desc_ok(const UnetrAugDesc* d) {
    if (!d || d->B <= 0 || d->num_samples <= 0 || d->B % d->num_samples) return false;
    if (d->C <= 0 || d->C > AUG_MAXC || d->L <= 0 || d->L > AUG_MAXC) return false;
    const int S[3] = {d->S0, d->S1, d->S2};
    for (int a = 0; a < 3; ++a) if (S[a] <= 0 || S[a] > AUG_MAXS) return false;
    if (d->ax0 < 0 || d->ax0 > 2 || d->ax1 < 0 || d->ax1 > 2 || d->ax0 == d->ax1 || S[d->ax0] != S[d->ax1]) return false;
    if (d->max_k <= 0 || d->B > 65535) return false;
    return d->sampling >= 0 && d->sampling <= 2;             // 2 (label classes) is drawn by unetr_aug_sample_classes alone
}

bool aug_affine_desc_ok(const UnetrAugAffineDesc* a) {
    if (!a || !(a->prob >= 0.0 && a->prob <= 1.0)) return false;
    for (int i = 0; i < 3; ++i) if (!(a->rotate[i] >= 0.0 && isfinite(a->rotate[i]))) return false;
    return a->zoom_lo > 0.0 && a->zoom_lo <= a->zoom_hi && isfinite(a->zoom_hi);
}

bool aug_intensity_desc_ok(const UnetrAugIntensityDesc* it) {
    if (!it) return false;
    for (int j = 0; j < 5; ++j) {
        if (!(it->prob[j] >= 0.0 && it->prob[j] <= 1.0)) return false;
        if (!(isfinite(it->lo[j]) && isfinite(it->hi[j]) && it->lo[j] <= it->hi[j])) return false;
        if (j == 0 ? it->lo[j] < 0.0 : it->lo[j] <= 0.0) return false;
    }
    return it->hi[1] <= 2.0;
}

// workspace of the intensity passes: [blur ping-pong, B C V floats][fp64 sums, B C nblk][mins][maxs]
inline size_t aug_intensity_tmp_bytes(const UnetrAugDesc* d) {
    const size_t n = (size_t)d->B * d->C * d->S0 * d->S1 * d->S2 * sizeof(float);
    return (n + 15) / 16 * 16;
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
    return unetr_check_launch();
}

extern "C" int unetr_aug_crop(const float* img, const float* lbl, int C, int L, int D, int H, int W, int z0, int y0, int x0,
                              int d, int h, int w, float* oimg, uint8_t* olbl, void* stream) {
    if (!img || !lbl || !oimg || !olbl || C <= 0 || L <= 0 || d <= 0 || h <= 0 || w <= 0 || z0 < 0 || y0 < 0 || x0 < 0 ||
        z0 + d > D || y0 + h > H || x0 + w > W || h > 65535 || (long)d * (C + L) > 65535)
        return UNETR_ERR_ARG;
    hipLaunchKernelGGL(aug_crop_kernel, dim3(cdiv(w, 256), h, d * (C + L)), dim3(256), 0, (hipStream_t)stream, img, lbl, C, L,
                       D, H, W, z0, y0, x0, d, h, w, oimg, olbl);
    return unetr_check_launch();
}

extern "C" int unetr_aug_index_count(const float* img, const uint8_t* lbl, int C, int L, long V, float thr, int* ws,
                                     size_t ws_ints, void* stream) {
    if (!img || !lbl || !ws || C <= 0 || L <= 0 || V <= 0 || V > 0x7fffffffL) return UNETR_ERR_ARG;
    if ((long)ws_ints < unetr_aug_index_ws_ints(V)) return UNETR_ERR_WORKSPACE;
    const int nblk = cdiv(V, AUG_CHUNK);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(aug_count_kernel<2>, dim3(nblk), dim3(256), 0, st, AugMember{img, lbl, C, L, 2, V, 0, thr}, ws, nblk);
    hipLaunchKernelGGL(aug_scan_kernel<int>, dim3(2), dim3(1024), 0, st, ws, nblk, ws + 4L * nblk);
    return unetr_check_launch();
}

extern "C" int unetr_aug_index_scatter(const float* img, const uint8_t* lbl, int C, int L, long V, float thr, const int* ws,
                                       size_t ws_ints, int* fg, int* bg, void* stream) {
    if (!img || !lbl || !ws || !fg || !bg || C <= 0 || L <= 0 || V <= 0 || V > 0x7fffffffL) return UNETR_ERR_ARG;
    if ((long)ws_ints < unetr_aug_index_ws_ints(V)) return UNETR_ERR_WORKSPACE;
    const int nblk = cdiv(V, AUG_CHUNK);
    hipLaunchKernelGGL(aug_scatter_kernel<2>, dim3(nblk), dim3(256), 0, (hipStream_t)stream, AugMember{img, lbl, C, L, 2, V, 0, thr},
                       ws, nblk, fg, bg, (const long long*)nullptr);
    return unetr_check_launch();
}

extern "C" long unetr_aug_class_ws_ints(long V, int K) {
    return V <= 0 || K < 1 || K > AUG_MAXK ? 0 : 2L * K * cdiv(V, AUG_CHUNK);
}

static bool aug_class_args_ok(const float* img, const uint8_t* lbl, int C, int L, int K, long V, int image_mask) {
    if (!lbl || (image_mask && !img) || C <= 0 || C > AUG_MAXC || L <= 0 || L > AUG_MAXC || V <= 0 || V > 0x7fffffffL) return false;
    return K >= 1 && K <= AUG_MAXK && (L == 1 || K == L);
}

extern "C" int unetr_aug_class_count(const float* img, const uint8_t* lbl, int C, int L, int K, long V, int image_mask, float thr,
                                     int* ws, size_t ws_ints, long long* offsets, void* stream) {
    if (!aug_class_args_ok(img, lbl, C, L, K, V, image_mask) || !ws || !offsets) return UNETR_ERR_ARG;
    if ((long)ws_ints < unetr_aug_class_ws_ints(V, K)) return UNETR_ERR_WORKSPACE;
    const int nblk = cdiv(V, AUG_CHUNK);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(aug_count_kernel<0>, dim3(nblk), dim3(256), 0, st, AugMember{img, lbl, C, L, K, V, image_mask, thr}, ws, nblk);
    hipLaunchKernelGGL(aug_scan_kernel<long long>, dim3(K), dim3(1024), 0, st, ws, nblk, offsets + 1);
    hipLaunchKernelGGL(aug_class_offsets_kernel, dim3(1), dim3(64), 0, st, offsets, K);
    return unetr_check_launch();
}

extern "C" int unetr_aug_class_scatter(const float* img, const uint8_t* lbl, int C, int L, int K, long V, int image_mask, float thr,
                                       const int* ws, size_t ws_ints, const long long* offsets, int* lists, void* stream) {
    if (!aug_class_args_ok(img, lbl, C, L, K, V, image_mask) || !ws || !offsets || !lists) return UNETR_ERR_ARG;
    if ((long)ws_ints < unetr_aug_class_ws_ints(V, K)) return UNETR_ERR_WORKSPACE;
    const int nblk = cdiv(V, AUG_CHUNK);
    hipLaunchKernelGGL(aug_scatter_kernel<0>, dim3(nblk), dim3(256), 0, (hipStream_t)stream,
                       AugMember{img, lbl, C, L, K, V, image_mask, thr}, ws, nblk, lists, (int*)nullptr, offsets);
    return unetr_check_launch();
}

extern "C" int unetr_aug_sample(const UnetrAugDesc* d, const long long* vols, int nvol, const int* order, long long* state,
                                int* params, void* stream) {
    if (!aug_desc_ok(d) || d->sampling == 2 || !vols || nvol <= 0 || !order || !state || !params) return UNETR_ERR_ARG;
    hipLaunchKernelGGL((aug_sample_kernel<false, false>), dim3(1), dim3(256), 0, (hipStream_t)stream, *d, UnetrAugAffineDesc{}, vols,
                       nvol, order, state, params, (float*)nullptr, AugClassArgs{});
    return unetr_check_launch();
}

extern "C" int unetr_aug_sample_affine(const UnetrAugDesc* d, const UnetrAugAffineDesc* a, const long long* vols, int nvol,
                                       const int* order, long long* state, int* params, float* affine, void* stream) {
    if (!aug_desc_ok(d) || d->sampling == 2 || !aug_affine_desc_ok(a) || !vols || nvol <= 0 || !order || !state || !params || !affine)
        return UNETR_ERR_ARG;
    hipLaunchKernelGGL((aug_sample_kernel<true, false>), dim3(1), dim3(256), 0, (hipStream_t)stream, *d, *a, vols, nvol, order, state,
                       params, affine, AugClassArgs{});
    return unetr_check_launch();
}

extern "C" int unetr_aug_sample_classes(const UnetrAugDesc* d, const UnetrAugAffineDesc* a, const long long* vols, int nvol,
                                        const long long* class_table, int K, const float* ratios, const int* order,
                                        long long* state, int* params, float* affine, int* classes, void* stream) {
    if (!aug_desc_ok(d) || d->sampling != 2 || !vols || nvol <= 0 || !class_table || K < 1 || K > AUG_MAXK || !ratios || !order ||
        !state || !params || !classes)
        return UNETR_ERR_ARG;
    if ((a != nullptr) != (affine != nullptr) || (a && !aug_affine_desc_ok(a))) return UNETR_ERR_ARG;
    const AugClassArgs cl{class_table, ratios, classes, K};
    if (a)
        hipLaunchKernelGGL((aug_sample_kernel<true, true>), dim3(1), dim3(256), 0, (hipStream_t)stream, *d, *a, vols, nvol, order,
                           state, params, affine, cl);
    else
        hipLaunchKernelGGL((aug_sample_kernel<false, true>), dim3(1), dim3(256), 0, (hipStream_t)stream, *d, UnetrAugAffineDesc{},
                           vols, nvol, order, state, params, (float*)nullptr, cl);
    return unetr_check_launch();
}

extern "C" size_t unetr_aug_gather_ws_bytes(const UnetrAugDesc* d) {
    if (!aug_desc_ok(d) || !d->normalize) return 0;
    const long V = (long)d->S0 * d->S1 * d->S2;
    return (size_t)d->B * d->C * cdiv(V, AUG_TILE) * 3 * sizeof(double);
}

// the gather over nblk workgroups per sample (affine: the table of aug_sample_kernel<true, .>, else null) and, with normalize, the
// pass that reduces its partials
static int aug_launch_gather(const UnetrAugDesc* d, const long long* vols, int nvol, const int* params, const float* affine, int nblk,
                             float* x, float* y, void* ws, hipStream_t st) {
    const dim3 grid(nblk, d->B);
    double* part = d->normalize ? (double*)ws : nullptr;
    if (d->normalize && affine) hipLaunchKernelGGL((aug_gather_kernel<true, true>), grid, dim3(256), 0, st, *d, vols, nvol, params, affine, x, y, part);
    else if (d->normalize) hipLaunchKernelGGL((aug_gather_kernel<true, false>), grid, dim3(256), 0, st, *d, vols, nvol, params, affine, x, y, part);
    else if (affine) hipLaunchKernelGGL((aug_gather_kernel<false, true>), grid, dim3(256), 0, st, *d, vols, nvol, params, affine, x, y, part);
    else hipLaunchKernelGGL((aug_gather_kernel<false, false>), grid, dim3(256), 0, st, *d, vols, nvol, params, affine, x, y, part);
    if (d->normalize)
        hipLaunchKernelGGL(aug_norm_kernel, dim3(AUG_NORM_WG, d->B * d->C), dim3(256), 0, st, x, (long)d->S0 * d->S1 * d->S2,
                           (const double*)ws, nblk);
    return unetr_check_launch();
}

extern "C" int unetr_aug_gather(const UnetrAugDesc* d, const long long* vols, int nvol, const int* params, float* x, float* y,
                                void* ws, size_t ws_bytes, void* stream) {
    if (!aug_desc_ok(d) || !vols || nvol <= 0 || !params || !x || !y) return UNETR_ERR_ARG;
    if (d->normalize && (!ws || ws_bytes < unetr_aug_gather_ws_bytes(d))) return UNETR_ERR_WORKSPACE;
    return aug_launch_gather(d, vols, nvol, params, nullptr, cdiv((long)d->S0 * d->S1 * d->S2, AUG_TILE), x, y, ws, (hipStream_t)stream);
}

extern "C" size_t unetr_aug_gather_affine_ws_bytes(const UnetrAugDesc* d) {
    if (!aug_desc_ok(d) || !d->normalize) return 0;
    return (size_t)d->B * d->C * aug_affine_blocks(d) * 3 * sizeof(double);
}

extern "C" int unetr_aug_gather_affine(const UnetrAugDesc* d, const long long* vols, int nvol, const int* params,
                                       const float* affine, float* x, float* y, void* ws, size_t ws_bytes, void* stream) {
    if (!aug_desc_ok(d) || !vols || nvol <= 0 || !params || !affine || !x || !y) return UNETR_ERR_ARG;
    if (d->normalize && (!ws || ws_bytes < unetr_aug_gather_affine_ws_bytes(d))) return UNETR_ERR_WORKSPACE;
    return aug_launch_gather(d, vols, nvol, params, affine, aug_affine_blocks(d), x, y, ws, (hipStream_t)stream);
}

extern "C" int unetr_aug_intensity_sample(const UnetrAugDesc* d, const UnetrAugIntensityDesc* it, const long long* state, int* table,
                                          void* stream) {
    if (!aug_desc_ok(d) || !aug_intensity_desc_ok(it) || !state || !table) return UNETR_ERR_ARG;
    hipLaunchKernelGGL(aug_intensity_sample_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, *d, *it, state, table);
    return unetr_check_launch();
}

extern "C" size_t unetr_aug_intensity_ws_bytes(const UnetrAugDesc* d) {
    if (!aug_desc_ok(d)) return 0;
    const long V = (long)d->S0 * d->S1 * d->S2;
    return aug_intensity_tmp_bytes(d) + (size_t)d->B * d->C * cdiv(V, AUG_TILE) * (sizeof(double) + 2 * sizeof(float));
}

extern "C" int unetr_aug_intensity_apply(const UnetrAugDesc* d, const int* table, float* x, void* ws, size_t ws_bytes, void* stream) {
    if (!aug_desc_ok(d) || !table || !x) return UNETR_ERR_ARG;
    if (!ws || ((size_t)ws & 15) || ws_bytes < unetr_aug_intensity_ws_bytes(d)) return UNETR_ERR_WORKSPACE;
    const long V = (long)d->S0 * d->S1 * d->S2;
    const int nblk = cdiv(V, AUG_TILE);
    const size_t parts = (size_t)d->B * d->C * nblk;
    float* tmp = (float*)ws;
    double* psum = (double*)((char*)ws + aug_intensity_tmp_bytes(d));
    float* pmin = (float*)(psum + parts);
    float* pmax = pmin + parts;
    hipStream_t st = (hipStream_t)stream;
    const long plane = (long)d->S1 * d->S2, rows = (long)d->C * d->S0 * d->S1;
    const int nr = std::max(1, AUG_BLUR_LDS / d->S2);
    // blur: axis 0 x -> tmp, axis 1 tmp -> x, axis 2 in place through LDS; then the two elementwise passes
    hipLaunchKernelGGL(aug_blur_strided_kernel, dim3(cdiv(d->C * plane, 256), cdiv(d->S0, AUG_BLUR_T), d->B), dim3(256), 0, st, table,
                       0, (const float*)x, tmp, (long)d->C * V, (long)d->C, d->S0, plane);
    hipLaunchKernelGGL(aug_blur_strided_kernel, dim3(cdiv((long)d->C * d->S0 * d->S2, 256), cdiv(d->S1, AUG_BLUR_T), d->B), dim3(256), 0,
                       st, table, 1, (const float*)tmp, x, (long)d->C * V, (long)d->C * d->S0, d->S1, (long)d->S2);
    hipLaunchKernelGGL(aug_blur_rows_kernel, dim3(cdiv(rows, nr), d->B), dim3(256), 0, st, table, (const float*)x, x, rows, d->S2, nr);
    hipLaunchKernelGGL(aug_intensity_point_kernel, dim3(nblk, d->C, d->B), dim3(256), 0, st, *d, table, x, psum, pmin, pmax);
    hipLaunchKernelGGL(aug_intensity_tone_kernel, dim3(cdiv(V, AUG_TONE_TILE), d->C, d->B), dim3(256), 0, st, *d, table, x, (const double*)psum,
                       (const float*)pmin, (const float*)pmax, nblk);
    return unetr_check_launch();
}
