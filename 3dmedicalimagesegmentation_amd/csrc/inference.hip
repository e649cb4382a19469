// Validation-side kernels around the forward pass (unetr_segmentation_3d.py:103-132): blending of sliding-window
// predictions (monai.inferers.sliding_window_inference, MONAI 0.6.0, called at :110) and the counts behind
// monai.metrics.DiceMetric on argmax / one-hot predictions (:405-406, :485-486, :118-125).  All HBM-bound streaming
// passes; the window forward itself is the training hot path run without autograd.
#include <algorithm>
#include "common.hpp"
#include "../../include/unetr_hip.h"

namespace {

// out[b, c, z0+z, y0+y, x0+x] += w(z,y,x) * seg[c, z, y, x];  count[b, z0+z, y0+y, x0+x] += w(z,y,x)
// One launch per window: windows of one volume overlap, and MONAI adds them in window order.
__global__ void __launch_bounds__(256)
sw_accumulate_kernel(const float* __restrict__ seg, const float* __restrict__ imp, float* __restrict__ out,
                     float* __restrict__ count, int C, int rz, int ry, int rx, int D, int H, int W, int z0, int y0, int x0) {
    const long rv = (long)rz * ry * rx, V = (long)D * H * W;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < rv; i += (long)gridDim.x * 256) {
        const int x = (int)(i % rx), y = (int)((i / rx) % ry), z = (int)(i / ((long)rx * ry));
        const long o = ((long)(z0 + z) * H + (y0 + y)) * W + (x0 + x);
        const float w = imp ? imp[i] : 1.f;
        for (int c = 0; c < C; ++c) out[(long)c * V + o] += w * seg[(long)c * rv + i];
        count[o] += w;
    }
}

__global__ void __launch_bounds__(256)
sw_finalize_kernel(float* __restrict__ out, const float* __restrict__ count, int B, int C, long V) {
    const long total = (long)B * C * V;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long v = i % V, b = i / ((long)C * V);
        out[i] = out[i] / count[b * V + v];
    }
}

// per (b, chunk): [C][3] partial sums of (pred * y, pred, y).  LOGITS: pred = one_hot(argmax_c logits) (first maximal
// channel, torch.argmax's rule) and y = one_hot(label ids); otherwise pred / y are taken as given ([B,C,V] each).
constexpr int DVPB = 4096;
constexpr int DMAXC = 16;
template <bool LOGITS>
__global__ void __launch_bounds__(256)
dice_counts_kernel(const float* __restrict__ pred, const float* __restrict__ y, int C, long V, float* __restrict__ part) {
    __shared__ float red[4][3 * DMAXC];
    const int b = blockIdx.y;
    const long v0 = (long)blockIdx.x * DVPB, v1 = std::min<long>(V, v0 + DVPB);
    float acc[3 * DMAXC];
    for (int k = 0; k < 3 * DMAXC; ++k) acc[k] = 0.f;
    for (long v = v0 + threadIdx.x; v < v1; v += 256) {
        if (LOGITS) {
            float mx = -3.0e38f;
            int am = 0;
            for (int c = 0; c < C; ++c) {
                const float z = pred[((long)b * C + c) * V + v];
                if (z > mx) { mx = z; am = c; }
            }
            const int lab = (int)y[(long)b * V + v];
#pragma unroll
            for (int c = 0; c < DMAXC; ++c) {
                if (c < C) {
                    const float p = c == am ? 1.f : 0.f, t = c == lab ? 1.f : 0.f;
                    acc[3 * c] += p * t; acc[3 * c + 1] += p; acc[3 * c + 2] += t;
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < DMAXC; ++c) {
                if (c < C) {
                    const float p = pred[((long)b * C + c) * V + v], t = y[((long)b * C + c) * V + v];
                    acc[3 * c] += p * t; acc[3 * c + 1] += p; acc[3 * c + 2] += t;
                }
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 3 * DMAXC; ++k) {
        const float s = wave_sum(acc[k]);
        if (lane == 0) red[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 3 * C)
        part[((long)b * gridDim.x + blockIdx.x) * (3 * C) + threadIdx.x] =
            red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

__global__ void __launch_bounds__(256)
dice_counts_final_kernel(const float* __restrict__ part, int BC3, int B, int C, int nchunk, double* __restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;     // index into [B][C][3]
    if (i >= BC3) return;
    const int b = i / (3 * C), k = i - b * 3 * C;
    double s = 0.0;
    for (int ch = 0; ch < nchunk; ++ch) s += (double)part[((long)b * nchunk + ch) * (3 * C) + k];
    counts[i] = s;
}

}  // namespace

extern "C" int unetr_sw_accumulate(const float* seg, const float* importance, float* out, float* count, int C,
                                   int rz, int ry, int rx, int D, int H, int W, int z0, int y0, int x0, void* stream) {
    if (!seg || !out || !count || C <= 0 || rz <= 0 || ry <= 0 || rx <= 0) return UNETR_ERR_ARG;
    if (z0 < 0 || y0 < 0 || x0 < 0 || z0 + rz > D || y0 + ry > H || x0 + rx > W) return UNETR_ERR_ARG;   // window inside the volume
    const long rv = (long)rz * ry * rx;
    const int blocks = (int)std::min<long>((rv + 255) / 256, 8192);
    hipLaunchKernelGGL(sw_accumulate_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, seg, importance, out, count, C, rz, ry, rx,
                       D, H, W, z0, y0, x0);
    return unetr_check_launch();
}

extern "C" int unetr_sw_finalize(float* out, const float* count, int B, int C, long V, void* stream) {
    if (!out || !count || B <= 0 || C <= 0 || V <= 0) return UNETR_ERR_ARG;
    const long total = (long)B * C * V;
    const int blocks = (int)std::min<long>((total + 255) / 256, 16384);
    hipLaunchKernelGGL(sw_finalize_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, out, count, B, C, V);
    return unetr_check_launch();
}

extern "C" int unetr_dice_counts(const float* pred, const float* y, int B, int C, long V, int from_logits, double* counts,
                                 float* ws, size_t ws_bytes, void* stream) {
    if (!pred || !y || !counts || B <= 0 || V <= 0 || B > 65535) return UNETR_ERR_ARG;
    if (C < 1 || C > DMAXC) return UNETR_ERR_UNSUPPORTED;
    const int nchunk = cdiv(V, DVPB);
    if (!ws || (size_t)B * nchunk * 3 * C * sizeof(float) > ws_bytes) return UNETR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (from_logits) hipLaunchKernelGGL(dice_counts_kernel<true>, dim3(nchunk, B), dim3(256), 0, st, pred, y, C, V, ws);
    else hipLaunchKernelGGL(dice_counts_kernel<false>, dim3(nchunk, B), dim3(256), 0, st, pred, y, C, V, ws);
    const int n = B * C * 3;
    hipLaunchKernelGGL(dice_counts_final_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, ws, n, B, C, nchunk, counts);
    return unetr_check_launch();
}

// ---- batched, table-driven sliding-window kernels (SlidingWindowInferer) ---------------------------------------------------
// One forward batch = one row of a device-resident window table; the volume (pointers, extents, padding) is described by a
// device-resident unetr_sw_volume, so none of these launches carries a volume size or a window position in its arguments and a
// hipGraph of advance -> gather -> forward -> accumulate serves every volume.  All three are HBM-bound streaming passes: four
// x-neighbours per thread, 16-byte accesses wherever the address is 16-byte aligned, plain vector stores, no atomics.
namespace {

constexpr int SWROW = UNETR_SW_ROW_INTS;

__device__ __forceinline__ bool sw_al16(const void* p) { return ((size_t)p & 15) == 0; }

template <int NV>
__device__ __forceinline__ void sw_ld(float (&r)[NV], const float* p) {
    if (NV == 4 && sw_al16(p)) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        r[0] = t.x; r[1 % NV] = t.y; r[2 % NV] = t.z; r[3 % NV] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < NV; ++k) r[k] = p[k];
    }
}

template <int NV>
__device__ __forceinline__ void sw_st(float* p, const float (&r)[NV]) {
    if (NV == 4 && sw_al16(p)) {
        *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1 % NV], r[2 % NV], r[3 % NV]);
    } else {
#pragma unroll
        for (int k = 0; k < NV; ++k) p[k] = r[k];
    }
}

// r[0..NV) in reverse order (the x-mirrored run of a window: load the mirrored aligned quad, reverse it in registers)
template <int NV>
__device__ __forceinline__ void sw_rev(float (&r)[NV]) {
#pragma unroll
    for (int k = 0; k < NV / 2; ++k) { const float t = r[k]; r[k] = r[NV - 1 - k]; r[NV - 1 - k] = t; }
}

// Window-local voxel (z, y, x .. x+NV-1) under flip mask f (bit 0 = z, 1 = y, 2 = x): the mirrored position.  With the x bit the
// result is the START of the mirrored run, which holds the NV voxels in reverse order.
__device__ __forceinline__ void sw_mirror(int f, int nv, int rz, int ry, int rx, int& z, int& y, int& x) {
    if (f & 1) z = rz - 1 - z;
    if (f & 2) y = ry - 1 - y;
    if (f & 4) x = rx - nv - x;
}

__global__ void sw_advance_kernel(unetr_sw_volume* vol) { vol->cursor = vol->cursor + 1; }
__global__ void sw_rewind_kernel(unetr_sw_volume* vol) { vol->cursor = -1; }

// the row in flight, or nullptr-like failure (uniform per launch): loads the row into LDS
__device__ __forceinline__ bool sw_load_row(const unetr_sw_volume* vol, int* row) {
    const int cur = vol->cursor;
    if (cur < 0 || cur >= vol->rows) return false;
    if (threadIdx.x < SWROW) row[threadIdx.x] = vol->table[(long)cur * SWROW + threadIdx.x];
    __syncthreads();
    return true;
}

// a slot is used only when its window lies inside the padded volume of an existing batch item (a bad table writes nothing)
__device__ __forceinline__ bool sw_slot_ok(const unetr_sw_volume* vol, const int* row, int i, int rz, int ry, int rx) {
    const int b = row[4 + 4 * i], z = row[5 + 4 * i], y = row[6 + 4 * i], x = row[7 + 4 * i];
    return b >= 0 && b < vol->B && z >= 0 && y >= 0 && x >= 0 && z + rz <= vol->D && y + ry <= vol->H && x + rx <= vol->W;
}

// dst[j, c, z, y, x] = in[b_j, c, z_j + z' - pz, y_j + y' - py, x_j + x' - px], cval outside the stored volume (and in unused slots);
// (z', y', x') = (z, y, x) mirrored inside the window along the axes of the row's flip mask (header int 1; 0: as they are).
template <int NV>
__global__ void __launch_bounds__(256)
sw_gather_batch_kernel(const unetr_sw_volume* __restrict__ vol, float* __restrict__ dst, int n, int Cin, int rz, int ry, int rx) {
    __shared__ int row[SWROW];
    if (vol->Cin != Cin || !sw_load_row(vol, row)) return;
    const int j = blockIdx.y;
    const int xq = rx / NV;
    const long rv = (long)rz * ry * rx, quads = (long)Cin * rz * ry * xq;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= quads) return;
    const int x = (int)(q % xq) * NV, y = (int)((q / xq) % ry), z = (int)((q / ((long)xq * ry)) % rz), c = (int)(q / ((long)xq * ry * rz));
    const float cval = vol->cval;
    float r[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) r[k] = cval;
    if (j < row[0] && sw_slot_ok(vol, row, j, rz, ry, rx)) {
        const int Di = vol->Di, Hi = vol->Hi, Wi = vol->Wi;
        const int f = row[1] & 7;
        int zs = z, ys = y, xs = x;
        sw_mirror(f, NV, rz, ry, rx, zs, ys, xs);
        const int Z = row[5 + 4 * j] + zs - vol->pz, Y = row[6 + 4 * j] + ys - vol->py, X = row[7 + 4 * j] + xs - vol->px;
        if (Z >= 0 && Z < Di && Y >= 0 && Y < Hi) {
            const float* src = vol->in + (((long)row[4 + 4 * j] * Cin + c) * Di + Z) * (long)Hi * Wi + (long)Y * Wi;
            if (X >= 0 && X + NV <= Wi) {
                sw_ld<NV>(r, src + X);
            } else {
#pragma unroll
                for (int k = 0; k < NV; ++k)
                    if (X + k >= 0 && X + k < Wi) r[k] = src[X + k];
            }
        }
        if (f & 4) sw_rev<NV>(r);
    }
    sw_st<NV>(dst + ((long)j * Cin + c) * rv + ((long)z * ry + y) * rx + x, r);
}

// NV x-neighbours at (Z, Y, X..) of one batch item, covered by exactly the windows in `mask`: add those windows in slot order.
// The per-window update is the one sw_accumulate_kernel performs (out = fma(w, seg, out); count = count + w), so a voxel
// receives the same fp32 operations in the same order as from one unetr_sw_accumulate launch per window.
// f: the row's flip mask -- the windows were forwarded mirrored, so seg is read at the mirrored position (the weight is not: it
// follows the position in the volume).  act: 0 seg as it is, 2 sigmoid(seg) per element, 1 softmax over the C channels of each
// covering window: one pass for max and sum (rescaled when the max moves), one that blends exp(s - max) / sum.
template <int NV>
__device__ __forceinline__ void sw_blend(const int* row, unsigned mask, int Z, int Y, int X, const float* __restrict__ seg,
                                         const float* __restrict__ imp, float* __restrict__ out, float* __restrict__ count,
                                         int C, int rz, int ry, int rx, long rv, int H, int W, long V, int f, int act) {
    const long o = ((long)Z * H + Y) * W + X;
    float cnt[NV], w[NV], s[NV], acc[NV];
    sw_ld<NV>(cnt, count + o);
    for (unsigned m = mask; m; m &= m - 1) {
        const int i = __ffs(m) - 1;
        const long li = ((long)(Z - row[5 + 4 * i]) * ry + (Y - row[6 + 4 * i])) * rx + (X - row[7 + 4 * i]);
        if (imp) sw_ld<NV>(w, imp + li);
#pragma unroll
        for (int k = 0; k < NV; ++k) cnt[k] += imp ? w[k] : 1.f;
    }
    sw_st<NV>(count + o, cnt);
    if (act == 1) {
        for (unsigned m = mask; m; m &= m - 1) {
            const int i = __ffs(m) - 1;
            int lz = Z - row[5 + 4 * i], ly = Y - row[6 + 4 * i], lx = X - row[7 + 4 * i];
            const long li = ((long)lz * ry + ly) * rx + lx;
            sw_mirror(f, NV, rz, ry, rx, lz, ly, lx);
            const float* ps = seg + (long)i * C * rv + ((long)lz * ry + ly) * rx + lx;
            if (imp) sw_ld<NV>(w, imp + li);
            float mx[NV], sum[NV];
            for (int c = 0; c < C; ++c) {
                sw_ld<NV>(s, ps + (long)c * rv);
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    if (c == 0) { mx[k] = s[k]; sum[k] = 1.f; }
                    else if (s[k] > mx[k]) { sum[k] = fmaf(sum[k], expf(mx[k] - s[k]), 1.f); mx[k] = s[k]; }
                    else sum[k] += expf(s[k] - mx[k]);
                }
            }
            for (int c = 0; c < C; ++c) {
                float* po = out + (long)c * V + o;
                sw_ld<NV>(s, ps + (long)c * rv);
#pragma unroll
                for (int k = 0; k < NV; ++k) s[k] = expf(s[k] - mx[k]) / sum[k];
                if (f & 4) sw_rev<NV>(s);
                sw_ld<NV>(acc, po);
#pragma unroll
                for (int k = 0; k < NV; ++k) acc[k] = fmaf(imp ? w[k] : 1.f, s[k], acc[k]);
                sw_st<NV>(po, acc);
            }
        }
        return;
    }
    for (int c = 0; c < C; ++c) {
        float* po = out + (long)c * V + o;
        sw_ld<NV>(acc, po);
        for (unsigned m = mask; m; m &= m - 1) {
            const int i = __ffs(m) - 1;
            int lz = Z - row[5 + 4 * i], ly = Y - row[6 + 4 * i], lx = X - row[7 + 4 * i];
            const long li = ((long)lz * ry + ly) * rx + lx;
            sw_mirror(f, NV, rz, ry, rx, lz, ly, lx);
            if (imp) sw_ld<NV>(w, imp + li);
            sw_ld<NV>(s, seg + ((long)i * C + c) * rv + ((long)lz * ry + ly) * rx + lx);
            if (f & 4) sw_rev<NV>(s);
            if (act == 2) {
#pragma unroll
                for (int k = 0; k < NV; ++k) s[k] = 1.f / (1.f + expf(-s[k]));
            }
#pragma unroll
            for (int k = 0; k < NV; ++k) acc[k] = fmaf(imp ? w[k] : 1.f, s[k], acc[k]);
        }
        sw_st<NV>(po, acc);
    }
}

// grid (tiles of window voxels, slot j).  The windows of one row overlap, so every output voxel has ONE owner: the thread of the
// first active slot that covers it.  The owner adds slot j, j+1, ... in order; every other thread leaves the voxel alone.
template <int NV>
__global__ void __launch_bounds__(256)
sw_accumulate_batch_kernel(const unetr_sw_volume* __restrict__ vol, const float* __restrict__ seg, const float* __restrict__ imp,
                           int n, int C, int rz, int ry, int rx) {
    __shared__ int row[SWROW];
    if (vol->C != C || !sw_load_row(vol, row)) return;
    const int j = blockIdx.y, nact = min(row[0], n);
    if (j >= nact || !sw_slot_ok(vol, row, j, rz, ry, rx)) return;
    const int xq = rx / NV;
    const long rv = (long)rz * ry * rx, quads = (long)rz * ry * xq;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= quads) return;
    const int b = row[4 + 4 * j];
    const int Z = row[5 + 4 * j] + (int)(q / ((long)xq * ry)), Y = row[6 + 4 * j] + (int)((q / xq) % ry), X = row[7 + 4 * j] + (int)(q % xq) * NV;
    unsigned mk[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) mk[k] = 0u;
    for (int i = 0; i < nact; ++i) {
        const int zi = row[5 + 4 * i], yi = row[6 + 4 * i], xi = row[7 + 4 * i];
        if (row[4 + 4 * i] != b || Z < zi || Z >= zi + rz || Y < yi || Y >= yi + ry || !sw_slot_ok(vol, row, i, rz, ry, rx)) continue;
#pragma unroll
        for (int k = 0; k < NV; ++k)
            if (X + k >= xi && X + k < xi + rx) mk[k] |= 1u << i;
    }
    const int H = vol->H, W = vol->W;
    const long V = (long)vol->D * H * W;
    float* out = vol->out + (long)b * C * V;
    float* count = vol->count + (long)b * V;
    const int f = row[1] & 7, act = vol->activation;
    bool same = true;
#pragma unroll
    for (int k = 1; k < NV; ++k) same = same && mk[k] == mk[0];
    if (NV > 1 && same) {
        if (__ffs(mk[0]) - 1 == j) sw_blend<NV>(row, mk[0], Z, Y, X, seg, imp, out, count, C, rz, ry, rx, rv, H, W, V, f, act);
        return;
    }
#pragma unroll
    for (int k = 0; k < NV; ++k)
        if (__ffs(mk[k]) - 1 == j) sw_blend<1>(row, mk[k], Z, Y, X + k, seg, imp, out, count, C, rz, ry, rx, rv, H, W, V, f, act);
}

// v = out / count, then per voxel: post 0 stores v; 1 stores one_hot(argmax_c v) over out; 2 stores argmax_c v (as float) into
// dst [B, V]; 3 stores (v >= thr) over out -- thr 0: sigmoid(v) >= 0.5 for blended logits; 0.5: for blended probabilities.  argmax
// takes the first maximal channel (torch.argmax).
template <int NV>
__global__ void __launch_bounds__(256)
sw_finalize_post_kernel(float* __restrict__ out, const float* __restrict__ count, float* __restrict__ dst, int C, long V, int post,
                        float thr) {
    const long v = ((long)blockIdx.x * 256 + threadIdx.x) * NV;
    if (v >= V) return;
    const int b = blockIdx.y;
    float cn[NV], a[NV], mx[NV];
    int am[NV];
    sw_ld<NV>(cn, count + (long)b * V + v);
    float* ob = out + (long)b * C * V + v;
    for (int c = 0; c < C; ++c) {
        sw_ld<NV>(a, ob + (long)c * V);
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            a[k] = a[k] / cn[k];
            if (c == 0 || a[k] > mx[k]) { mx[k] = a[k]; am[k] = c; }
            if (post == 3) a[k] = a[k] >= thr ? 1.f : 0.f;
        }
        if (post == 0 || post == 3) sw_st<NV>(ob + (long)c * V, a);
    }
    if (post == 1) {
        for (int c = 0; c < C; ++c) {
#pragma unroll
            for (int k = 0; k < NV; ++k) a[k] = am[k] == c ? 1.f : 0.f;
            sw_st<NV>(ob + (long)c * V, a);
        }
    } else if (post == 2) {
#pragma unroll
        for (int k = 0; k < NV; ++k) a[k] = (float)am[k];
        sw_st<NV>(dst + (long)b * V + v, a);
    }
}

}  // namespace

extern "C" int unetr_sw_advance(unetr_sw_volume* vol, void* stream) {
    if (!vol) return UNETR_ERR_ARG;
    hipLaunchKernelGGL(sw_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, vol);
    return unetr_check_launch();
}

extern "C" int unetr_sw_rewind(unetr_sw_volume* vol, void* stream) {
    if (!vol) return UNETR_ERR_ARG;
    hipLaunchKernelGGL(sw_rewind_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, vol);
    return unetr_check_launch();
}

extern "C" int unetr_sw_gather_batch(const unetr_sw_volume* vol, float* dst, int n, int Cin, int rz, int ry, int rx, void* stream) {
    if (!vol || !dst || Cin <= 0 || rz <= 0 || ry <= 0 || rx <= 0) return UNETR_ERR_ARG;
    if (n < 1 || n > UNETR_SW_MAX_BATCH) return UNETR_ERR_UNSUPPORTED;
    const bool v4 = rx % 4 == 0 && ((size_t)dst & 15) == 0;
    const long quads = (long)Cin * rz * ry * (rx / (v4 ? 4 : 1));
    const dim3 grid(cdiv(quads, 256), n);
    if (v4) hipLaunchKernelGGL(sw_gather_batch_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, vol, dst, n, Cin, rz, ry, rx);
    else hipLaunchKernelGGL(sw_gather_batch_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, vol, dst, n, Cin, rz, ry, rx);
    return unetr_check_launch();
}

extern "C" int unetr_sw_accumulate_batch(const unetr_sw_volume* vol, const float* seg, const float* importance, int n, int C,
                                         int rz, int ry, int rx, void* stream) {
    if (!vol || !seg || C <= 0 || rz <= 0 || ry <= 0 || rx <= 0) return UNETR_ERR_ARG;
    if (n < 1 || n > UNETR_SW_MAX_BATCH) return UNETR_ERR_UNSUPPORTED;
    const bool v4 = rx % 4 == 0 && ((size_t)seg & 15) == 0 && ((size_t)importance & 15) == 0;
    const long quads = (long)rz * ry * (rx / (v4 ? 4 : 1));
    const dim3 grid(cdiv(quads, 256), n);
    hipStream_t st = (hipStream_t)stream;
    if (v4) hipLaunchKernelGGL(sw_accumulate_batch_kernel<4>, grid, dim3(256), 0, st, vol, seg, importance, n, C, rz, ry, rx);
    else hipLaunchKernelGGL(sw_accumulate_batch_kernel<1>, grid, dim3(256), 0, st, vol, seg, importance, n, C, rz, ry, rx);
    return unetr_check_launch();
}

extern "C" int unetr_sw_finalize_post_thr(float* out, const float* count, float* dst, int B, int C, long V, int post, float threshold,
                                          void* stream) {
    if (!out || !count || B <= 0 || B > 65535 || C <= 0 || V <= 0 || post < 0 || post > 3 || (post == 2 && !dst)) return UNETR_ERR_ARG;
    if ((post == 1 || post == 2) && C > DMAXC) return UNETR_ERR_UNSUPPORTED;
    const bool v4 = V % 4 == 0 && ((size_t)out & 15) == 0 && ((size_t)count & 15) == 0 && ((size_t)dst & 15) == 0;
    const dim3 grid(cdiv(cdiv(V, v4 ? 4 : 1), 256), B);
    hipStream_t st = (hipStream_t)stream;
    if (v4) hipLaunchKernelGGL(sw_finalize_post_kernel<4>, grid, dim3(256), 0, st, out, count, dst, C, V, post, threshold);
    else hipLaunchKernelGGL(sw_finalize_post_kernel<1>, grid, dim3(256), 0, st, out, count, dst, C, V, post, threshold);
    return unetr_check_launch();
}

extern "C" int unetr_sw_finalize_post(float* out, const float* count, float* dst, int B, int C, long V, int post, void* stream) {
    return unetr_sw_finalize_post_thr(out, count, dst, B, C, V, post, 0.f, stream);
}
