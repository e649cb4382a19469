// Per-volume front of the reference's transform chain on the GPU: Spacingd(pixdim, mode=("bilinear",
// "nearest")) -> Orientationd(axcodes) [-> ConvertToMultiChannelBasedOnBratsClassesd on the label] of
// unetr_segmentation_3d.py:326-331 as ONE gather.  Both transforms are affine maps on voxel indices, so the host
// (preprocess.plan) folds them into a 3x4 matrix and every output voxel j reads the source at clamp(mat @ [j, 1], 0, n - 1):
// trilinear for the image, round-half-even nearest for the label (MONAI 0.6.0 semantics as restated in tests/preprocess_ref.py).
//
//   pre_resample_kernel   one workgroup = one compact output brick of 1024 voxels (x fastest), so its source footprint is a small
//                         box whichever axes the orientation swaps; one thread = 4 voxels along x.
//                         Source coordinates in fp64 (label picks must agree with the float64 reference), once per voxel;
//                         then the C image channels (fp32 weights and blend, 16-byte stores) and the label bytes in the same
//                         pass.  An all-integer matrix (identity spacing: a pure flip / transpose) takes the one-tap path
//                         for the image too and returns the input values bit for bit.
#include <math.h>
#include <stdint.h>
#include "resample.hpp"
#include "../../include/unetr_hip.h"

namespace {

constexpr int PRE_MAXC = 8;                   // image channels / label channels, as VolumeCache

struct PreMat { double m[12]; };              // row a: source index along input axis a = m[4a .. 4a+2] . (j0, j1, j2) + m[4a+3]

__device__ __forceinline__ float pre_ld(const float* p, long i) { return p[i]; }
__device__ __forceinline__ float pre_ld(const int16_t* p, long i) { return (float)p[i]; }

template <typename SrcT, bool NEAREST, int BX, int BY, int BZ>
__global__ __launch_bounds__(256) void pre_resample_kernel(const SrcT* __restrict__ img, const uint8_t* __restrict__ lbl, int C,
                                                           int L, int brats, int n0, int n1, int n2, PreMat M, int D, int H,
                                                           int W, float* __restrict__ oimg, uint8_t* __restrict__ olbl,
                                                           int vec_ok) {
    int y, z;
    long o;
    if (!rs_brick_row<BX, BY, BZ>(D, H, W, y, z, o)) return;
    const int x0 = blockIdx.x * BX + (threadIdx.x % (BX / RS_VPT)) * RS_VPT - (int)(o & 3);      // the lane owns 4 consecutive voxels
    if (x0 >= W) return;
    const bool full = vec_ok && x0 >= 0 && x0 + RS_VPT <= W;

    const long s1 = n2, s0 = (long)n1 * n2, Vin = s0 * n0;
    int onear[RS_VPT];                        // nearest source voxel
    RsTaps tp;
#pragma unroll
    for (int k = 0; k < RS_VPT; ++k) {
        // every coordinate is clamped into the source, so the loads of a voxel off the row's ends (never stored) stay in bounds
        const double j0 = (double)z, j1 = (double)y, j2 = (double)(x0 + k);
        const double p0 = fmin(fmax(rs_affine_row(M.m, 0, j0, j1, j2), 0.0), (double)(n0 - 1));
        const double p1 = fmin(fmax(rs_affine_row(M.m, 1, j0, j1, j2), 0.0), (double)(n1 - 1));
        const double p2 = fmin(fmax(rs_affine_row(M.m, 2, j0, j1, j2), 0.0), (double)(n2 - 1));
        onear[k] = (int)((long)rint(p0) * s0 + (long)rint(p1) * s1 + (long)rint(p2));
        if (!NEAREST) rs_taps(tp, k, p0, p1, p2, n0, n1, n2, s0, s1);
    }

    const long Vout = (long)D * H * W;
    for (int c = 0; c < C; ++c) {
        const SrcT* src = img + c * Vin;
        float v[RS_VPT];
#pragma unroll
        for (int k = 0; k < RS_VPT; ++k) v[k] = NEAREST ? pre_ld(src, onear[k]) : rs_trilinear(src, tp, k);
        rs_store_group(oimg, c * Vout, o, x0, W, full, v);
    }
    if (!lbl) return;
    for (int l = 0; l < L; ++l) {
        uint8_t b[RS_VPT];
#pragma unroll
        for (int k = 0; k < RS_VPT; ++k) {
            if (brats) {      // ConvertToMultiChannelBasedOnBratsClassesd: background, TC = 2|3, WT = 1|2|3, ET = 3
                const uint8_t u = lbl[onear[k]];
                b[k] = l == 0 ? u == 0 : l == 1 ? (u == 2 || u == 3) : l == 2 ? (u >= 1 && u <= 3) : u == 3;
            } else {
                b[k] = lbl[l * Vin + onear[k]];
            }
        }
        rs_store_group(olbl, l * Vout, o, x0, W, full, b);
    }
}

struct PreArgs {
    const void* img; const uint8_t* lbl; int C, L, brats, n0, n1, n2; PreMat M; int D, H, W; float* oimg; uint8_t* olbl; int vec_ok;
};

template <typename SrcT, bool NEAREST>
int pre_launch(int axis, const PreArgs& a, hipStream_t st) {
    RS_BRICK_DISPATCH(axis, a.D, a.H, a.W,
                      hipLaunchKernelGGL((pre_resample_kernel<SrcT, NEAREST, BX, BY, BZ>), grid, dim3(256), 0, st, (const SrcT*)a.img,
                                         a.lbl, a.C, a.L, a.brats, a.n0, a.n1, a.n2, a.M, a.D, a.H, a.W, a.oimg, a.olbl, a.vec_ok));
}

}  // namespace

extern "C" int unetr_resample_orient(const void* img, int img_int16, const unsigned char* lbl, int C, int L, int brats, int n0,
                                     int n1, int n2, const double* mat, int D, int H, int W, float* oimg, unsigned char* olbl,
                                     void* stream) {
    if (!img || !mat || !oimg || (lbl && !olbl) || n0 <= 0 || n1 <= 0 || n2 <= 0 || D <= 0 || H <= 0 || W <= 0) return UNETR_ERR_ARG;
    if (C < 1 || C > PRE_MAXC || (lbl && (L < 1 || L > PRE_MAXC || (brats && L != 4)))) return UNETR_ERR_ARG;
    if ((long)n0 * n1 * n2 > 0x7fffffffL || (long)D * H * W > 0x7fffffffL) return UNETR_ERR_UNSUPPORTED;
    const RsMatrix ms = rs_scan_matrix(mat);
    if (!ms.finite) return UNETR_ERR_ARG;
    PreArgs a{img, lbl, C, L, brats, n0, n1, n2, {}, D, H, W, oimg, olbl, 0};
    for (int i = 0; i < 12; ++i) a.M.m[i] = mat[i];
    a.vec_ok = ((uintptr_t)oimg & 15) == 0 && (!lbl || ((uintptr_t)olbl & 3) == 0);
    hipStream_t st = (hipStream_t)stream;
    if (img_int16) return ms.integer ? pre_launch<int16_t, true>(ms.axis, a, st) : pre_launch<int16_t, false>(ms.axis, a, st);
    return ms.integer ? pre_launch<float, true>(ms.axis, a, st) : pre_launch<float, false>(ms.axis, a, st);
}
