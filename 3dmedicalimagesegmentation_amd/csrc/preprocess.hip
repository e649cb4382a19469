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
#include "common.hpp"
#include "../../include/unetr_hip.h"

namespace {

constexpr int PRE_VPT = 4;                    // voxels per thread along x: one float4 / one packed uchar4 store
constexpr int PRE_MAXC = 8;                   // image channels / label channels, as VolumeCache

struct PreMat { double m[12]; };              // row a: source index along input axis a = m[4a .. 4a+2] . (j0, j1, j2) + m[4a+3]

__device__ __forceinline__ float pre_ld(const float* p, long i) { return p[i]; }
__device__ __forceinline__ float pre_ld(const int16_t* p, long i) { return (float)p[i]; }

// a + t * (b - a) as two fmas: exact at t = 0 and t = 1, and the same instructions for every source type and channel count
__device__ __forceinline__ float pre_lerp(float a, float b, float t) { return fmaf(t, b, fmaf(-t, a, a)); }

template <typename SrcT, bool NEAREST, int BX, int BY, int BZ>
__global__ __launch_bounds__(256) void pre_resample_kernel(const SrcT* __restrict__ img, const uint8_t* __restrict__ lbl, int C,
                                                           int L, int brats, int n0, int n1, int n2, PreMat M, int D, int H,
                                                           int W, float* __restrict__ oimg, uint8_t* __restrict__ olbl,
                                                           int vec_ok) {
    constexpr int TX = BX / PRE_VPT;
    static_assert(BX % PRE_VPT == 0 && TX * BY * BZ == 256, "a brick is 256 threads x 4 voxels");
    const int t = threadIdx.x;
    const int y = blockIdx.y * BY + (t / TX) % BY;
    const int z = blockIdx.z * BZ + t / (TX * BY);
    if (y >= H || z >= D) return;
    // rows start at any element offset (W is arbitrary), so the 4-voxel groups are shifted left by the row's offset mod 4: every
    // group that lies inside the row is then one aligned 16-byte (image) / 4-byte (label) store, only the row ends go voxel by voxel
    const long o = ((long)z * H + y) * W;
    const int x0 = blockIdx.x * BX + (t % TX) * PRE_VPT - (int)(o & 3);
    if (x0 >= W) return;
    const bool full = vec_ok && x0 >= 0 && x0 + PRE_VPT <= W;

    const long s1 = n2, s0 = (long)n1 * n2, Vin = s0 * n0;
    int onear[PRE_VPT];                       // nearest source voxel
    int obase[PRE_VPT], dz[PRE_VPT], dy[PRE_VPT], dx[PRE_VPT];   // trilinear: low corner and the (clamped) steps to the high one
    float tz[PRE_VPT], ty[PRE_VPT], tx[PRE_VPT];
#pragma unroll
    for (int k = 0; k < PRE_VPT; ++k) {
        // every coordinate is clamped into the source, so the loads of a voxel off the row's ends (never stored) stay in bounds
        const double j0 = (double)z, j1 = (double)y, j2 = (double)(x0 + k);
        double s[3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
            s[a] = fma(M.m[4 * a], j0, fma(M.m[4 * a + 1], j1, fma(M.m[4 * a + 2], j2, M.m[4 * a + 3])));
        s[0] = fmin(fmax(s[0], 0.0), (double)(n0 - 1));
        s[1] = fmin(fmax(s[1], 0.0), (double)(n1 - 1));
        s[2] = fmin(fmax(s[2], 0.0), (double)(n2 - 1));
        onear[k] = (int)((long)rint(s[0]) * s0 + (long)rint(s[1]) * s1 + (long)rint(s[2]));
        if (!NEAREST) {
            const double f0 = floor(s[0]), f1 = floor(s[1]), f2 = floor(s[2]);
            const int i0 = (int)f0, i1 = (int)f1, i2 = (int)f2;
            tz[k] = (float)(s[0] - f0); ty[k] = (float)(s[1] - f1); tx[k] = (float)(s[2] - f2);
            obase[k] = (int)(i0 * s0 + i1 * s1 + i2);
            dz[k] = i0 + 1 < n0 ? (int)s0 : 0;
            dy[k] = i1 + 1 < n1 ? (int)s1 : 0;
            dx[k] = i2 + 1 < n2 ? 1 : 0;
        }
    }

    const long Vout = (long)D * H * W;
    for (int c = 0; c < C; ++c) {
        const SrcT* src = img + c * Vin;
        float v[PRE_VPT];
#pragma unroll
        for (int k = 0; k < PRE_VPT; ++k) {
            if (NEAREST) {
                v[k] = pre_ld(src, onear[k]);
            } else {
                const long b = obase[k];
                const float a000 = pre_ld(src, b), a001 = pre_ld(src, b + dx[k]);
                const float a010 = pre_ld(src, b + dy[k]), a011 = pre_ld(src, b + dy[k] + dx[k]);
                const float a100 = pre_ld(src, b + dz[k]), a101 = pre_ld(src, b + dz[k] + dx[k]);
                const float a110 = pre_ld(src, b + dz[k] + dy[k]), a111 = pre_ld(src, b + dz[k] + dy[k] + dx[k]);
                const float l00 = pre_lerp(a000, a001, tx[k]), l01 = pre_lerp(a010, a011, tx[k]);
                const float l10 = pre_lerp(a100, a101, tx[k]), l11 = pre_lerp(a110, a111, tx[k]);
                v[k] = pre_lerp(pre_lerp(l00, l01, ty[k]), pre_lerp(l10, l11, ty[k]), tz[k]);
            }
        }
        float* dst = oimg + c * Vout + o + x0;
        if (full && ((c * Vout) & 3) == 0) {
            *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int k = 0; k < PRE_VPT; ++k)
                if (x0 + k >= 0 && x0 + k < W) dst[k] = v[k];
        }
    }
    if (!lbl) return;
    for (int l = 0; l < L; ++l) {
        uint8_t b[PRE_VPT];
#pragma unroll
        for (int k = 0; k < PRE_VPT; ++k) {
            if (brats) {      // ConvertToMultiChannelBasedOnBratsClassesd: background, TC = 2|3, WT = 1|2|3, ET = 3
                const uint8_t u = lbl[onear[k]];
                b[k] = l == 0 ? u == 0 : l == 1 ? (u == 2 || u == 3) : l == 2 ? (u >= 1 && u <= 3) : u == 3;
            } else {
                b[k] = lbl[l * Vin + onear[k]];
            }
        }
        uint8_t* dst = olbl + l * Vout + o + x0;
        if (full && ((l * Vout) & 3) == 0) {
            *reinterpret_cast<uchar4*>(dst) = make_uchar4(b[0], b[1], b[2], b[3]);
        } else {
#pragma unroll
            for (int k = 0; k < PRE_VPT; ++k)
                if (x0 + k >= 0 && x0 + k < W) dst[k] = b[k];
        }
    }
}

struct PreArgs {
    const void* img; const uint8_t* lbl; int C, L, brats, n0, n1, n2; PreMat M; int D, H, W; float* oimg; uint8_t* olbl; int vec_ok;
};

template <typename SrcT, bool NEAREST, int BX, int BY, int BZ>
int pre_launch_brick(const PreArgs& a, hipStream_t st) {
    const long gx = cdiv(a.W + PRE_VPT - 1, BX), gy = cdiv(a.H, BY), gz = cdiv(a.D, BZ);    // + 3: the shifted groups
    if (gy > 65535 || gz > 65535) return UNETR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL((pre_resample_kernel<SrcT, NEAREST, BX, BY, BZ>), dim3(gx, gy, gz), dim3(256), 0, st, (const SrcT*)a.img,
                       a.lbl, a.C, a.L, a.brats, a.n0, a.n1, a.n2, a.M, a.D, a.H, a.W, a.oimg, a.olbl, a.vec_ok);
    return hipGetLastError() == hipSuccess ? UNETR_OK : UNETR_ERR_LAUNCH;
}

// axis = the output axis along which the source's fastest axis changes most: the brick (x, y, z output voxels, 1024 per workgroup)
// is long on it, so that a workgroup reads whole cache lines of the source whichever way the orientation turns the volume.
// DESIGN.md section 13 lists the shapes that were timed and what was not.
template <typename SrcT, bool NEAREST>
int pre_launch(int axis, const PreArgs& a, hipStream_t st) {
    if (axis == 2) return pre_launch_brick<SrcT, NEAREST, 64, 4, 4>(a, st);
    if (axis == 1) return pre_launch_brick<SrcT, NEAREST, 16, 8, 8>(a, st);
    return pre_launch_brick<SrcT, NEAREST, 16, 4, 16>(a, st);
}

}  // namespace

extern "C" int unetr_resample_orient(const void* img, int img_int16, const unsigned char* lbl, int C, int L, int brats, int n0,
                                     int n1, int n2, const double* mat, int D, int H, int W, float* oimg, unsigned char* olbl,
                                     void* stream) {
    if (!img || !mat || !oimg || (lbl && !olbl) || n0 <= 0 || n1 <= 0 || n2 <= 0 || D <= 0 || H <= 0 || W <= 0) return UNETR_ERR_ARG;
    if (C < 1 || C > PRE_MAXC || (lbl && (L < 1 || L > PRE_MAXC || (brats && L != 4)))) return UNETR_ERR_ARG;
    if ((long)n0 * n1 * n2 > 0x7fffffffL || (long)D * H * W > 0x7fffffffL) return UNETR_ERR_UNSUPPORTED;
    PreArgs a{img, lbl, C, L, brats, n0, n1, n2, {}, D, H, W, oimg, olbl, 0};
    bool integer = true;
    for (int i = 0; i < 12; ++i) {
        if (!isfinite(mat[i])) return UNETR_ERR_ARG;
        a.M.m[i] = mat[i];
        integer = integer && mat[i] == rint(mat[i]);
    }
    a.vec_ok = ((uintptr_t)oimg & 15) == 0 && (!lbl || ((uintptr_t)olbl & 3) == 0);
    int axis = 2;                                  // row 2 of mat = the source's fastest axis
    for (int j = 0; j < 2; ++j)
        if (fabs(mat[8 + j]) > fabs(mat[8 + axis])) axis = j;
    hipStream_t st = (hipStream_t)stream;
    if (img_int16) return integer ? pre_launch<int16_t, true>(axis, a, st) : pre_launch<int16_t, false>(axis, a, st);
    return integer ? pre_launch<float, true>(axis, a, st) : pre_launch<float, false>(axis, a, st);
}
