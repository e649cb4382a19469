// What the two resampling gathers share (preprocess.hip: raw scan -> working grid; restore.hip: prediction ->
// the scan's own grid, section 17).  Both cut the output into compact bricks of 1024 voxels, one thread = 4 voxels along x, take every
// output voxel through a 3x4 matrix in fp64 to a clamped source position, read one tap or eight there and store 4-voxel groups.
// Every multiply-add is an explicit fma / fmaf, so the compiler has nothing left to contract and both files get the same bits.
// What differs on purpose stays in the files: preprocess's lanes own four consecutive voxels, restore's lanes load strided voxels
// and exchange them inside the quad (section 17 has the A/B); the crop box, the post-processing, the label channels.
// The augment gather's fp32 arithmetic (aug_affine_taps / aug_trilinear, pinned by tests/augment_affine_ref.py) is another one.
#pragma once
#include <math.h>
#include <stdint.h>
#include "common.hpp"

constexpr int RS_VPT = 4;                     // voxels per thread along x: one 16-byte (float) / 4-byte (byte) store

// a + t * (b - a) as two fmas: exact at t = 0 and t = 1, and the same instructions for every source type and channel count
__device__ __forceinline__ float rs_lerp(float a, float b, float t) { return fmaf(t, b, fmaf(-t, a, a)); }

// row a of the 3x4 matrix m at the output index (j0, j1, j2): the source position along input axis a, fp64
__device__ __forceinline__ double rs_affine_row(const double* m, int a, double j0, double j1, double j2) {
    return fma(m[4 * a], j0, fma(m[4 * a + 1], j1, fma(m[4 * a + 2], j2, m[4 * a + 3])));
}

// the eight taps of each of a thread's RS_VPT voxels: low corner, the (clamped) steps to the high one, the fractions
struct RsTaps { int base[RS_VPT], dz[RS_VPT], dy[RS_VPT], dx[RS_VPT]; float tz[RS_VPT], ty[RS_VPT], tx[RS_VPT]; };

// voxel k at p, a position already clamped into the source [n0][n1][n2] (strides s0, s1, 1), so every tap stays in bounds
__device__ __forceinline__ void rs_taps(RsTaps& t, int k, double p0, double p1, double p2, int n0, int n1, int n2, long s0, long s1) {
    const double f0 = floor(p0), f1 = floor(p1), f2 = floor(p2);
    const int i0 = (int)f0, i1 = (int)f1, i2 = (int)f2;
    t.tz[k] = (float)(p0 - f0); t.ty[k] = (float)(p1 - f1); t.tx[k] = (float)(p2 - f2);
    t.base[k] = (int)(i0 * s0 + i1 * s1 + i2);
    t.dz[k] = i0 + 1 < n0 ? (int)s0 : 0;
    t.dy[k] = i1 + 1 < n1 ? (int)s1 : 0;
    t.dx[k] = i2 + 1 < n2 ? 1 : 0;
}

// trilinear value of voxel k in one channel: fp32 weights and blend, x then y then z
template <typename SrcT>
__device__ __forceinline__ float rs_trilinear(const SrcT* src, const RsTaps& t, int k) {
    const long b = t.base[k];
    const float a000 = (float)src[b], a001 = (float)src[b + t.dx[k]];
    const float a010 = (float)src[b + t.dy[k]], a011 = (float)src[b + t.dy[k] + t.dx[k]];
    const float a100 = (float)src[b + t.dz[k]], a101 = (float)src[b + t.dz[k] + t.dx[k]];
    const float a110 = (float)src[b + t.dz[k] + t.dy[k]], a111 = (float)src[b + t.dz[k] + t.dy[k] + t.dx[k]];
    const float l00 = rs_lerp(a000, a001, t.tx[k]), l01 = rs_lerp(a010, a011, t.tx[k]);
    const float l10 = rs_lerp(a100, a101, t.tx[k]), l11 = rs_lerp(a110, a111, t.tx[k]);
    return rs_lerp(rs_lerp(l00, l01, t.ty[k]), rs_lerp(l10, l11, t.ty[k]), t.tz[k]);
}

// The thread's row of its brick (BX x BY x BZ output voxels of a [D][H][W] grid): y, z and the row's element offset o; false when
// the row lies outside the grid.  Rows start at any element offset (W is arbitrary), so callers shift the 4-voxel groups left by
// o & 3: every group inside the row is then one aligned vector store, only the row ends go voxel by voxel.
template <int BX, int BY, int BZ>
__device__ __forceinline__ bool rs_brick_row(int D, int H, int W, int& y, int& z, long& o) {
    constexpr int TX = BX / RS_VPT;
    static_assert(BX % RS_VPT == 0 && TX * BY * BZ == 256, "a brick is 256 threads x 4 voxels");
    const int t = threadIdx.x;
    y = blockIdx.y * BY + (t / TX) % BY;
    z = blockIdx.z * BZ + t / (TX * BY);
    o = ((long)z * H + y) * W;
    return y < H && z < D;
}

__device__ __forceinline__ void rs_store4(float* dst, const float* v) {
    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void rs_store4(uint8_t* dst, const uint8_t* v) {
    *reinterpret_cast<uchar4*>(dst) = make_uchar4(v[0], v[1], v[2], v[3]);
}

// the 4-voxel group from x0 of one channel plane (float or byte): an aligned vector store inside the row (full: the group lies in
// [0, W) and the buffer is aligned), voxel by voxel at the row's ends and in a plane that starts off the vector boundary
template <typename T>
__device__ __forceinline__ void rs_store_group(T* out, long chan_off, long o, int x0, int W, bool full, const T* v) {
    T* dst = out + chan_off + o + x0;
    if (full && (chan_off & 3) == 0) {
        rs_store4(dst, v);
    } else {
#pragma unroll
        for (int k = 0; k < RS_VPT; ++k)
            if (x0 + k >= 0 && x0 + k < W) dst[k] = v[k];
    }
}

// ---------------------------------------------------------------- host
// the 12 matrix entries: all finite; all integers (a pure flip / transpose: the one-tap path returns the source's bits); axis = the
// output axis along which the source's fastest axis (row 2) changes most
struct RsMatrix { bool finite, integer; int axis; };
static inline RsMatrix rs_scan_matrix(const double* m) {
    RsMatrix r{true, true, 2};
    for (int i = 0; i < 12; ++i) {
        r.finite = r.finite && isfinite(m[i]);
        r.integer = r.integer && m[i] == rint(m[i]);
    }
    for (int j = 0; j < 2; ++j)
        if (fabs(m[8 + j]) > fabs(m[8 + r.axis])) r.axis = j;
    return r;
}

// Run the launch statement with BX, BY, BZ bound to the brick chosen by `axis` and `grid` to its grid over a [D][H][W] output, then
// return the launch status.  The brick is long on `axis`, so that a workgroup reads whole cache lines of the source whichever way the
// volume is turned (DESIGN.md section 13 lists the shapes that were timed).
#define RS_BRICK_(bx, by, bz, D, H, W, ...)                                                             \
    {                                                                                                   \
        constexpr int BX = bx, BY = by, BZ = bz;                                                        \
        const long gx = cdiv((W) + RS_VPT - 1, BX), gy = cdiv(H, BY), gz = cdiv(D, BZ); /* + 3: the shifted groups */ \
        if (gy > 65535 || gz > 65535) return UNETR_ERR_UNSUPPORTED;                                     \
        const dim3 grid(gx, gy, gz);                                                                    \
        __VA_ARGS__;                                                                                    \
        return unetr_check_launch();                                                                    \
    }
#define RS_BRICK_DISPATCH(axis, D, H, W, ...)                           \
    do {                                                                \
        if ((axis) == 2) RS_BRICK_(64, 4, 4, D, H, W, __VA_ARGS__)      \
        else if ((axis) == 1) RS_BRICK_(16, 8, 8, D, H, W, __VA_ARGS__) \
        else RS_BRICK_(16, 4, 16, D, H, W, __VA_ARGS__)                 \
    } while (0)
