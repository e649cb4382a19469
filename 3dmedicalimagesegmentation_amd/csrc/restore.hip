// The way back from the 1 mm RAS working grid to a scan's own voxel grid: the inverse of
// Spacingd -> Orientationd -> CropForegroundd (MONAI 0.6.0's Spacingd.inverse / Orientationd.inverse / CropForegroundd.inverse as
// restated in tests/restore_ref.py) as ONE gather, the twin of csrc/preprocess.hip: what the two share is csrc/resample.hpp.  The host (preprocess.Geometry) inverts the
// forward 4x4, so every NATIVE voxel i reads the prediction, which lives on the foreground crop of the resampled grid, at
//
//     s = clamp(Minv @ [i, 1], 0, full - 1)        border padding on the un-spaced grid, fp64
//     r = rint(s)                                   half to even; r outside the crop box on any axis: BACKGROUND, every output 0
//     nearest: src[r - origin]      linear: trilinear at clamp(s - origin, 0, crop - 1), i.e. with the taps clamped into the box
//
//   restore_kernel   one workgroup = one compact brick of 1024 native voxels (x fastest), one thread = 4 voxels along x, groups
//                    shifted by the row offset mod 4 so that a group inside a row is one aligned 16-byte (float) / 4-byte (byte)
//                    store -- the layout of pre_resample_kernel, except that a lane LOADS the voxels lx, lx + TX, ... of its
//                    row segment and a 4x4 exchange inside each quad of lanes puts 4 consecutive voxels into one lane for the
//                    store.  Coordinates once per voxel, then the C source channels in one pass: stored as they are (post 0),
//                    reduced to a running (best, index) over the channels (argmax: the C-channel volume on the native grid is
//                    never stored), thresholded (sigmoid: logit >= 0), and optionally folded into the BraTS label map.  An
//                    all-integer matrix (a scan that was copied forward: a pure flip / transpose) takes the one-tap path and
//                    returns the source's bits.
#include <math.h>
#include <stdint.h>
#include "resample.hpp"
#include "../../include/unetr_hip.h"

namespace {

constexpr int RST_MAXC = 16;                  // source channels, as unetr_sw_finalize_post's argmax
enum { RST_POST_NONE = 0, RST_POST_ARGMAX = 1, RST_POST_SIGMOID = 2 };

__device__ __forceinline__ float rst_zero(float) { return 0.f; }
__device__ __forceinline__ uint8_t rst_zero(uint8_t) { return 0; }

// Loads want consecutive lanes on consecutive voxels (lane lx reads voxels xb + lx + TX * k: a wave-wide load then touches the
// fewest cache lines whatever the source's step; DESIGN.md section 17 has the A/B), stores want 4 consecutive voxels per lane.
// For every k the 4 lanes of a quad hold 4 consecutive voxels, so one 4x4 transpose inside the quad (4 shuffles) turns the first
// layout into the second: lane r receives from lane j its value k = r, out[j] = (lane j).v[r], and then owns the k = r group.
// Every lane of a quad shares y and z and the row test on xb, so all four are active here.
template <typename T>
__device__ __forceinline__ T rst_sel4(const T* v, int i) { return i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : v[3]; }
__device__ __forceinline__ float rst_shfl4(float v, int lane) { return __shfl(v, lane, 4); }
__device__ __forceinline__ uint8_t rst_shfl4(uint8_t v, int lane) { return (uint8_t)__shfl((int)v, lane, 4); }

template <typename T>
__device__ __forceinline__ void rst_quad_transpose(T* v, int r) {
    T out[RS_VPT];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int j = (r - d) & 3;                                   // lane j sends its v[(j + d) & 3] = v[r of the receiver]
        const T got = rst_shfl4(rst_sel4(v, (r + d) & 3), j);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e == j) out[e] = got;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = out[e];
}

// one 4-voxel group of one output channel, v in the load layout
template <typename T>
__device__ __forceinline__ void rst_put(T* plane, long chan_off, long o, int x0, int W, bool full, int r, T* v) {
    rst_quad_transpose(v, r);
    rs_store_group(plane, chan_off, o, x0, W, full, v);
}

// SrcT float / uint8_t.  NEAREST: one tap per voxel (mode nearest, or an all-integer matrix).  post / brats are uniform over the
// launch.  The output is SrcT [C] planes when post == 0 && !brats, else bytes: [1] (argmax, brats) or [C] (sigmoid).
template <typename SrcT, bool NEAREST, int BX, int BY, int BZ>
__global__ __launch_bounds__(256) void restore_kernel(const SrcT* __restrict__ src, int C, unetr_restore_geom G, int N0, int N1,
                                                      int N2, int post, int brats, void* __restrict__ out, int vec_ok) {
    constexpr int TX = BX / RS_VPT;
    int y, z;
    long o;
    if (!rs_brick_row<BX, BY, BZ>(N0, N1, N2, y, z, o)) return;
    const int lx = threadIdx.x % TX, ql = lx & 3;                  // lane along x, and its place in its quad
    const int xb = blockIdx.x * BX - (int)(o & 3);               // the row's first (shifted) group of this brick
    if (xb >= N2) return;
    // loads: voxel k of this lane is xb + lx + TX * k.  stores (after the quad transpose): the 4 voxels from x0
    const int x0 = xb + RS_VPT * ((TX / 4) * ql + (lx >> 2));
    const bool full = vec_ok && x0 >= 0 && x0 + RS_VPT <= N2;

    const int c0 = G.crop[0], c1 = G.crop[1], c2 = G.crop[2];
    const long s1 = c2, s0 = (long)c1 * c2, Vin = s0 * c0;
    bool in[RS_VPT];                          // rint(s) lies inside the crop box
    int onear[RS_VPT];                        // nearest source voxel (0 for a background voxel: loaded, never used)
    RsTaps tp;
#pragma unroll
    for (int k = 0; k < RS_VPT; ++k) {
        // every source index below is clamped into the crop, so the loads of a voxel off the row's ends (never stored) and of a
        // background voxel (replaced by 0) stay in bounds
        const double i0 = (double)z, i1 = (double)y, i2 = (double)(xb + lx + TX * k);
        double s[3];
        long r[3];
        bool inside = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            s[a] = fmin(fmax(rs_affine_row(G.m, a, i0, i1, i2), 0.0), (double)(G.full[a] - 1));
            r[a] = (long)rint(s[a]) - G.origin[a];
            inside = inside && r[a] >= 0 && r[a] < G.crop[a];
        }
        in[k] = inside;
        onear[k] = inside ? (int)(r[0] * s0 + r[1] * s1 + r[2]) : 0;
        if (!NEAREST) {
            const double p0 = fmin(fmax(s[0] - G.origin[0], 0.0), (double)(c0 - 1));
            const double p1 = fmin(fmax(s[1] - G.origin[1], 0.0), (double)(c1 - 1));
            const double p2 = fmin(fmax(s[2] - G.origin[2], 0.0), (double)(c2 - 1));
            rs_taps(tp, k, p0, p1, p2, c0, c1, c2, s0, s1);
        }
    }

    const long Vout = (long)N0 * N1 * N2;
    const bool bytes_out = post != RST_POST_NONE || brats;
    float best[RS_VPT];
    int arg[RS_VPT];
    unsigned set[RS_VPT];                     // bit c: channel c of the discrete result is set (brats)
#pragma unroll
    for (int k = 0; k < RS_VPT; ++k) { best[k] = 0.f; arg[k] = 0; set[k] = 0u; }

    for (int c = 0; c < C; ++c) {
        const SrcT* sc = src + c * Vin;
        SrcT v[RS_VPT];
#pragma unroll
        for (int k = 0; k < RS_VPT; ++k) {
            if constexpr (NEAREST) v[k] = sc[onear[k]];
            else v[k] = rs_trilinear(sc, tp, k);
            if (!in[k]) v[k] = rst_zero(v[k]);            // a select, never a product: a NaN outside the box stays outside
        }
        if (!bytes_out) {
            rst_put<SrcT>((SrcT*)out, c * Vout, o, x0, N2, full, ql, v);
            continue;
        }
        uint8_t bit[RS_VPT];
#pragma unroll
        for (int k = 0; k < RS_VPT; ++k) {
            const float f = (float)v[k];
            if (c == 0 || f > best[k]) { best[k] = f; arg[k] = c; }      // first maximal channel, as unetr_sw_finalize_post
            bit[k] = post == RST_POST_SIGMOID ? (in[k] && f >= 0.f) : (f == 1.f);
            set[k] |= (unsigned)bit[k] << c;
        }
        if (post == RST_POST_SIGMOID && !brats) rst_put<uint8_t>((uint8_t*)out, c * Vout, o, x0, N2, full, ql, bit);
    }
    if (!bytes_out || (post == RST_POST_SIGMOID && !brats)) return;
    uint8_t b[RS_VPT];
#pragma unroll
    for (int k = 0; k < RS_VPT; ++k) {
        if (post == RST_POST_ARGMAX) set[k] = in[k] ? 1u << arg[k] : 0u;
        // channels BG / TC / WT / ET -> 1 where WT, then 2 where TC, then 3 where ET: the later rule wins
        b[k] = brats ? ((set[k] & 8u) ? 3 : (set[k] & 2u) ? 2 : (set[k] & 4u) ? 1 : 0) : (uint8_t)(in[k] ? arg[k] : 0);
    }
    rst_put<uint8_t>((uint8_t*)out, 0, o, x0, N2, full, ql, b);
}

struct RstArgs { const void* src; int C; unetr_restore_geom G; int n0, n1, n2, post, brats; void* out; int vec_ok; };

// the brick shapes are the ones DESIGN.md section 13 timed for the forward gather (not re-timed per shape here: section 17)
template <typename SrcT, bool NEAREST>
int rst_launch(int axis, const RstArgs& a, hipStream_t st) {
    RS_BRICK_DISPATCH(axis, a.n0, a.n1, a.n2,
                      hipLaunchKernelGGL((restore_kernel<SrcT, NEAREST, BX, BY, BZ>), grid, dim3(256), 0, st, (const SrcT*)a.src, a.C,
                                         a.G, a.n0, a.n1, a.n2, a.post, a.brats, a.out, a.vec_ok));
}

}  // namespace

extern "C" int unetr_restore_native(const void* src, int src_u8, int C, unetr_restore_geom g, int n0, int n1, int n2, int linear,
                                    int post, int brats, void* out, void* stream) {
    if (!src || !out || n0 <= 0 || n1 <= 0 || n2 <= 0 || C < 1 || C > RST_MAXC) return UNETR_ERR_ARG;
    if (post < RST_POST_NONE || post > RST_POST_SIGMOID || (post && !linear) || (src_u8 && linear)) return UNETR_ERR_ARG;
    if (brats && (C != 4 || (linear && !post))) return UNETR_ERR_ARG;
    long vfull = 1;
    for (int a = 0; a < 3; ++a) {
        if (g.full[a] <= 0 || g.crop[a] <= 0 || g.origin[a] < 0 || (long)g.origin[a] + g.crop[a] > g.full[a]) return UNETR_ERR_ARG;
        vfull *= g.full[a];
        if (vfull > 0x7fffffffL) return UNETR_ERR_UNSUPPORTED;                    // the box lies inside the grid: no more voxels
    }
    if ((long)n0 * n1 * n2 > 0x7fffffffL) return UNETR_ERR_UNSUPPORTED;
    const RsMatrix ms = rs_scan_matrix(g.m);
    if (!ms.finite) return UNETR_ERR_ARG;
    const bool bytes_out = post || brats || src_u8;
    RstArgs a{src, C, g, n0, n1, n2, post, brats, out, ((uintptr_t)out & (bytes_out ? 3 : 15)) == 0};
    hipStream_t st = (hipStream_t)stream;
    if (src_u8) return rst_launch<uint8_t, true>(ms.axis, a, st);
    return (!linear || ms.integer) ? rst_launch<float, true>(ms.axis, a, st) : rst_launch<float, false>(ms.axis, a, st);
}
