// Binary morphology on bit-packed masks and hole filling (scipy.ndimage.binary_dilation / _erosion / _opening / _closing /
// binary_fill_holes; the fill_holes rule of MONAI restated in DESIGN.md section 22).
//
// A *plane* is one [D, H, W] mask.  Packed, a row of W voxels is nw = ceil(W / 64) 64-bit words, bit b of word w = voxel
// x = 64 w + b; the bits at x >= W of a row's last word are never trusted: the step overwrites them with the border value when
// it loads a word and unpack does not look at them.
//
//   pack     one wave = one 64-voxel x segment of one row (the segmenting of ccl_init_kernel), four segments per wave; the word
//            is the wave's __ballot
//   step     k <= MORPH_K iterations of dilation (OR) or erosion (AND) in LDS: a workgroup owns MORPH_T x MORPH_T whole rows,
//            loads them with a halo of k rows in z and y, and ping-pongs between two LDS images; the region that is still
//            exact shrinks by one row per iteration and ends as the tile.  Erosion runs as the dilation of the complement
//            (words and border inverted on load, inverted back on store), so there is one word formula per connectivity
//   unpack   0 / 1 in the caller's dtype; contour = m & ~erode(m) of two packed images in the same pass
//   fill     three kernels over the label map unetr_ccl made of the background: faces -> flag[root], neighbour ids -> ids[root]
//            (class-id maps), apply
//
// Stream-ordered launches on fixed grids, integer atomics only, no host synchronisation: every call can be captured in a graph.
#include "common.hpp"

namespace {

constexpr int MORPH_T = 8;                         // tile: rows along z and along y
constexpr int MORPH_K = 4;                         // iterations fused in one launch = rows of halo on each side
constexpr int MORPH_HALO = MORPH_T + 2 * MORPH_K;  // 16 x 16 rows x nw <= 16 words x 8 B = 32 KiB per image, two images
constexpr int MORPH_SEGS = 4;                      // 64-voxel segments per wave in pack and unpack
constexpr int MORPH_MAXC = 16;
constexpr int MORPH_MAXN = 1024;
constexpr int MORPH_MAX_PLANES = 65535;            // grid.y / grid.z

enum { MORPH_DILATE = 0, MORPH_ERODE = 1, MORPH_OPEN = 2, MORPH_CLOSE = 3, MORPH_CONTOUR = 4 };

struct MorphShape {
    int D, H, W, nw;
    long V, S;                                     // voxels, 64-voxel segments per plane
};

// one wave = one 64-voxel x segment of one row at a time, MORPH_SEGS consecutive segments (= consecutive packed words) per wave
// with their loads issued together; false past the last segment (wave-uniform)
__device__ __forceinline__ bool morph_segment(const MorphShape& P, long s, int lane, int& x, long& v) {
    if (s >= P.S) return false;
    x = (int)(s % P.nw) * 64 + lane;
    v = (s / P.nw) * P.W + x;
    return true;
}

// class_id < 0: bit = in != 0; else bit = in == class_id (a class-id map, as edt.hip derives its masks)
template <class T>
__global__ __launch_bounds__(256) void morph_pack_kernel(const T* __restrict__ in, MorphShape P, int class_id,
                                                         unsigned long long* __restrict__ packed) {
    const int lane = threadIdx.x & 63;
    const long s0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * MORPH_SEGS;
    const T* ip = in + (size_t)blockIdx.y * P.V;
    T f[MORPH_SEGS];
#pragma unroll
    for (int j = 0; j < MORPH_SEGS; ++j) {
        int x;
        long v;
        f[j] = (T)0;
        if (morph_segment(P, s0 + j, lane, x, v) && x < P.W) {
            f[j] = ip[v];
            if (class_id >= 0) f[j] = (T)(f[j] == (T)class_id);
        }
    }
    unsigned long long mine = 0;
#pragma unroll
    for (int j = 0; j < MORPH_SEGS; ++j) {
        const unsigned long long m = __ballot(f[j] != (T)0);
        if (lane == j) mine = m;
    }
    if (lane < MORPH_SEGS && s0 + lane < P.S) packed[(size_t)blockIdx.y * P.S + s0 + lane] = mine;
}

// out = bit of a, or of a & ~b when b is given (the contour: a = the mask, b = its erosion)
template <class T>
__global__ __launch_bounds__(256) void morph_unpack_kernel(const unsigned long long* __restrict__ a,
                                                           const unsigned long long* __restrict__ b, MorphShape P,
                                                           T* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long s0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * MORPH_SEGS;
    const size_t wbase = (size_t)blockIdx.y * P.S;
    T* op = out + (size_t)blockIdx.y * P.V;
#pragma unroll
    for (int j = 0; j < MORPH_SEGS; ++j) {
        int x;
        long v;
        if (!morph_segment(P, s0 + j, lane, x, v)) break;
        if (x >= P.W) continue;
        unsigned long long m = a[wbase + s0 + j];
        if (b) m &= ~b[wbase + s0 + j];
        op[v] = (T)((m >> lane) & 1ull);
    }
}

// The rows of word w around haloed row (lz, ly) of an LDS image, split by how scipy's generate_binary_structure(3, CONN) treats
// them: `xd` is x-dilated by the caller, `plain` is taken as it is.
//   CONN 1: xd = centre row;                       plain = the four rows with |dz| + |dy| == 1
//   CONN 2: xd = centre row | those four rows;     plain = the four diagonal rows
//   CONN 3: xd = all nine rows;                    plain = nothing
template <int CONN>
__device__ __forceinline__ void morph_rows(const unsigned long long* img, int c, int nw, unsigned long long& xd,
                                           unsigned long long& plain) {
    const int sy = nw, sz = MORPH_HALO * nw;
    const unsigned long long axis = img[c - sy] | img[c + sy] | img[c - sz] | img[c + sz];
    xd = img[c];
    plain = 0;
    if (CONN == 1) { plain = axis; return; }
    xd |= axis;
    const unsigned long long diag = img[c - sz - sy] | img[c - sz + sy] | img[c + sz - sy] | img[c + sz + sy];
    if (CONN == 2) plain = diag;
    else xd |= diag;
}

template <int CONN>
__global__ __launch_bounds__(256) void morph_step_kernel(const unsigned long long* __restrict__ src,
                                                         unsigned long long* __restrict__ dst, MorphShape P, int k, int erode,
                                                         int border) {
    extern __shared__ unsigned long long morph_lds[];
    const int nw = P.nw;
    unsigned long long* cur = morph_lds;
    unsigned long long* nxt = morph_lds + MORPH_HALO * MORPH_HALO * nw;
    const int z0 = blockIdx.y * MORPH_T - MORPH_K, y0 = blockIdx.x * MORPH_T - MORPH_K;      // volume row of haloed row 0
    const size_t plane = (size_t)blockIdx.z * P.S;
    // working polarity: erosion is the dilation of the complement under the complemented border
    const unsigned long long flip = erode ? ~0ull : 0ull;
    const unsigned long long fill = (border ? ~0ull : 0ull) ^ flip;
    const unsigned long long tail = (P.W & 63) ? ~0ull >> (64 - (P.W & 63)) : ~0ull;         // bits of the last word with x < W
    int lo = MORPH_K - k, side = MORPH_T + 2 * k;      // haloed rows [lo, lo + side) along z and y are exact
    for (int t = threadIdx.x; t < side * side * nw; t += 256) {
        const int w = t % nw, r = t / nw, lz = lo + r / side, ly = lo + r % side;
        const int z = z0 + lz, y = y0 + ly;
        unsigned long long v = fill;
        if (z >= 0 && z < P.D && y >= 0 && y < P.H) {
            v = src[plane + ((size_t)z * P.H + y) * nw + w] ^ flip;
            if (w == nw - 1) v = (v & tail) | (fill & ~tail);
        }
        cur[(lz * MORPH_HALO + ly) * nw + w] = v;
    }
    __syncthreads();
    for (int i = 0; i < k; ++i) {
        lo += 1;
        side -= 2;
        for (int t = threadIdx.x; t < side * side * nw; t += 256) {
            const int w = t % nw, r = t / nw, lz = lo + r / side, ly = lo + r % side;
            const int z = z0 + lz, y = y0 + ly, c = (lz * MORPH_HALO + ly) * nw + w;
            unsigned long long v = fill;                 // rows outside the volume stay at the border value
            if (z >= 0 && z < P.D && y >= 0 && y < P.H) {
                unsigned long long xd, plain, l = fill, rr = fill, unused;
                morph_rows<CONN>(cur, c, nw, xd, plain);
                if (w > 0) morph_rows<CONN>(cur, c - 1, nw, l, unused);
                if (w + 1 < nw) morph_rows<CONN>(cur, c + 1, nw, rr, unused);
                v = plain | xd | (xd << 1) | (l >> 63) | (xd >> 1) | (rr << 63);
                if (w == nw - 1) v = (v & tail) | (fill & ~tail);
            }
            nxt[c] = v;
        }
        __syncthreads();
        unsigned long long* const sw = cur; cur = nxt; nxt = sw;
    }
    for (int t = threadIdx.x; t < MORPH_T * MORPH_T * nw; t += 256) {
        const int w = t % nw, r = t / nw, lz = MORPH_K + r / MORPH_T, ly = MORPH_K + r % MORPH_T;
        const int z = z0 + lz, y = y0 + ly;
        if (z < P.D && y < P.H) dst[plane + ((size_t)z * P.H + y) * nw + w] = cur[(lz * MORPH_HALO + ly) * nw + w] ^ flip;
    }
}

// ---- hole filling over the canonical labels (1 + smallest linear index) unetr_ccl gave the background's components

// flag[label - 1] = 1 for every labelled voxel on one of the six faces (byte stores of the same value: no atomics needed)
__global__ __launch_bounds__(256) void fill_faces_kernel(const int* __restrict__ labels, int D, int H, int W, long V,
                                                         uint8_t* __restrict__ flag) {
    int t = blockIdx.x * 256 + threadIdx.x;
    const int fz = H * W, fy = D * W, fx = D * H;
    int z, y, x;
    if (t < 2 * fz) { z = t < fz ? 0 : D - 1; t %= fz; y = t / W; x = t % W; }
    else if ((t -= 2 * fz) < 2 * fy) { y = t < fy ? 0 : H - 1; t %= fy; z = t / W; x = t % W; }
    else if ((t -= 2 * fy) < 2 * fx) { x = t < fx ? 0 : W - 1; t %= fx; z = t / H; y = t % H; }
    else return;
    const size_t base = (size_t)blockIdx.y * V;
    const int lab = labels[base + ((size_t)z * H + y) * W + x];
    if (lab) flag[base + lab - 1] = 1;
}

// class id of a voxel of a class-id map as a bit: 1 << id for integral ids 1..31, bit 0 for any other non-zero value
template <class T>
__device__ __forceinline__ unsigned fill_id_bit(T f) {
    if (f == (T)0) return 0u;
    const float g = (float)f;
    if (!(g >= 1.f && g <= 31.f) || g != (float)(int)g) return 1u;
    return 1u << (int)g;
}

// ids[label - 1] |= the id bits of the non-background voxels among the structure neighbours of every background voxel
template <class T, int CONN>
__global__ __launch_bounds__(256) void fill_neighbours_kernel(const T* __restrict__ in, const int* __restrict__ labels, int D,
                                                              int H, int W, long V, unsigned* __restrict__ ids) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const size_t base = (size_t)blockIdx.y * V;
    const int lab = labels[base + v];
    if (!lab) return;
    const int x = (int)(v % W), y = (int)(v / W % H), z = (int)(v / ((long)W * H));
    unsigned m = 0;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if ((dz != 0) + (dy != 0) + (dx != 0) > CONN) continue;
                const int zz = z + dz, yy = y + dy, xx = x + dx;
                if (zz < 0 || zz >= D || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                m |= fill_id_bit(in[base + ((size_t)zz * H + yy) * W + xx]);
            }
    if (m) atomicOr(ids + base + lab - 1, m);
}

// binary (ids == NULL): out = in != 0 || hole;  class-id map: out = hole bordered by exactly one applied id ? that id : in
template <class T>
__global__ __launch_bounds__(256) void fill_apply_kernel(const T* __restrict__ in, const int* __restrict__ labels, long V,
                                                         const uint8_t* __restrict__ flag, const unsigned* __restrict__ ids,
                                                         unsigned applied, T* __restrict__ out) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const size_t base = (size_t)blockIdx.y * V;
    const T f = in[base + v];
    const int lab = labels[base + v];
    const bool hole = lab != 0 && !flag[base + lab - 1];
    if (!ids) { out[base + v] = (T)(f != (T)0 || hole); return; }
    T o = f;
    if (hole) {
        const unsigned m = ids[base + lab - 1];
        if (__popc(m) == 1 && (m & applied)) o = (T)(__ffs((int)m) - 1);
    }
    out[base + v] = o;
}

inline size_t morph_al256(size_t x) { return (x + 255) & ~(size_t)255; }

bool morph_shape_ok(int D, int H, int W) {
    return D <= MORPH_MAXN && H <= MORPH_MAXN && W <= MORPH_MAXN && (long)D * H * W < 2147483647L;
}

MorphShape morph_shape(int D, int H, int W) {
    MorphShape P;
    P.D = D; P.H = H; P.W = W;
    P.nw = cdiv(W, 64);
    P.V = (long)D * H * W;
    P.S = (long)D * H * P.nw;
    return P;
}

// n iterations of one operation: ceil(n / MORPH_K) launches that alternate between the two packed images; returns the image
// that holds the result
unsigned long long* morph_iterate(unsigned long long* a, unsigned long long* b, const MorphShape& P, int N, int n, int erode,
                                  int connectivity, int border, hipStream_t st) {
    const dim3 grid(cdiv(P.H, MORPH_T), cdiv(P.D, MORPH_T), N);
    const size_t lds = (size_t)2 * MORPH_HALO * MORPH_HALO * P.nw * sizeof(unsigned long long);
    for (int done = 0; done < n; done += MORPH_K) {
        const int k = std::min(MORPH_K, n - done);
        if (connectivity == 1) hipLaunchKernelGGL(morph_step_kernel<1>, grid, dim3(256), lds, st, a, b, P, k, erode, border);
        else if (connectivity == 2) hipLaunchKernelGGL(morph_step_kernel<2>, grid, dim3(256), lds, st, a, b, P, k, erode, border);
        else hipLaunchKernelGGL(morph_step_kernel<3>, grid, dim3(256), lds, st, a, b, P, k, erode, border);
        std::swap(a, b);
    }
    return a;
}

template <class T>
int morph_run(const T* in, T* out, const MorphShape& P, int N, int class_id, int op, int iterations, int connectivity, int border,
              unsigned long long* a, unsigned long long* b, hipStream_t st) {
    const dim3 seg(cdiv(P.S, 4 * MORPH_SEGS), N);
    hipLaunchKernelGGL(morph_pack_kernel<T>, seg, dim3(256), 0, st, in, P, class_id, a);
    const unsigned long long *res, *minus = nullptr;
    if (op == MORPH_OPEN || op == MORPH_CLOSE) {      // scipy: both halves with border_value 0
        unsigned long long* mid = morph_iterate(a, b, P, N, iterations, op == MORPH_OPEN, connectivity, 0, st);
        res = morph_iterate(mid, mid == a ? b : a, P, N, iterations, op == MORPH_CLOSE, connectivity, 0, st);
    } else if (op == MORPH_CONTOUR) {
        res = a;
        minus = morph_iterate(a, b, P, N, 1, 1, connectivity, 0, st);
    } else {
        res = morph_iterate(a, b, P, N, iterations, op == MORPH_ERODE, connectivity, border, st);
    }
    hipLaunchKernelGGL(morph_unpack_kernel<T>, seg, dim3(256), 0, st, res, minus, P, out);
    return unetr_check_launch();
}

template <class T>
int fill_run(const T* in, T* out, const int* labels, int N, int D, int H, int W, int class_map, unsigned applied, int connectivity,
             uint8_t* flag, unsigned* ids, hipStream_t st) {
    const long V = (long)D * H * W;
    const long faces = 2L * ((long)H * W + (long)D * W + (long)D * H);
    hipLaunchKernelGGL(fill_faces_kernel, dim3(cdiv(faces, 256), N), dim3(256), 0, st, labels, D, H, W, V, flag);
    const dim3 vox(cdiv(V, 256), N);
    if (class_map) {
        if (connectivity == 1) hipLaunchKernelGGL((fill_neighbours_kernel<T, 1>), vox, dim3(256), 0, st, in, labels, D, H, W, V, ids);
        else if (connectivity == 2) hipLaunchKernelGGL((fill_neighbours_kernel<T, 2>), vox, dim3(256), 0, st, in, labels, D, H, W, V, ids);
        else hipLaunchKernelGGL((fill_neighbours_kernel<T, 3>), vox, dim3(256), 0, st, in, labels, D, H, W, V, ids);
    }
    hipLaunchKernelGGL(fill_apply_kernel<T>, vox, dim3(256), 0, st, in, labels, V, flag, class_map ? ids : nullptr, applied, out);
    return unetr_check_launch();
}

}  // namespace

extern "C" size_t unetr_morph_workspace_bytes(int D, int H, int W, int N) {
    if (D <= 0 || H <= 0 || W <= 0 || N <= 0 || N > MORPH_MAX_PLANES || !morph_shape_ok(D, H, W)) return 0;
    return 2 * morph_al256((size_t)N * morph_shape(D, H, W).S * sizeof(unsigned long long));
}

extern "C" int unetr_morph(const void* in, void* out, int u8, int B, int C, int D, int H, int W, int class_id, int op,
                           int iterations, int connectivity, int border_value, void* ws, size_t ws_bytes, void* stream) {
    if (!in || !out || !ws || B <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0) return UNETR_ERR_ARG;
    if (op < MORPH_DILATE || op > MORPH_CONTOUR || iterations < 1 || connectivity < 1 || connectivity > 3 || border_value < 0 ||
        border_value > 1 || class_id > 255)
        return UNETR_ERR_ARG;
    if (C > MORPH_MAXC || !morph_shape_ok(D, H, W) || (long)B * C > MORPH_MAX_PLANES) return UNETR_ERR_UNSUPPORTED;
    const int N = B * C;
    const size_t need = unetr_morph_workspace_bytes(D, H, W, N);
    if (need > ws_bytes) return UNETR_ERR_WORKSPACE;
    const MorphShape P = morph_shape(D, H, W);
    unsigned long long* a = (unsigned long long*)ws;
    unsigned long long* b = (unsigned long long*)((char*)ws + need / 2);
    hipStream_t st = (hipStream_t)stream;
    if (u8) return morph_run((const uint8_t*)in, (uint8_t*)out, P, N, class_id, op, iterations, connectivity, border_value, a, b, st);
    return morph_run((const float*)in, (float*)out, P, N, class_id, op, iterations, connectivity, border_value, a, b, st);
}

extern "C" size_t unetr_fill_holes_workspace_bytes(int D, int H, int W, int N, int class_map) {
    if (D <= 0 || H <= 0 || W <= 0 || N <= 0 || N > MORPH_MAX_PLANES || !morph_shape_ok(D, H, W)) return 0;
    return morph_al256((size_t)N * D * H * W * (class_map ? 5 : 1));
}

extern "C" int unetr_fill_holes(const void* in, void* out, int u8, const int* labels, int B, int C, int D, int H, int W,
                                int class_map, unsigned applied, int connectivity, void* ws, size_t ws_bytes, void* stream) {
    if (!in || !out || !labels || !ws || B <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0) return UNETR_ERR_ARG;
    if (connectivity < 1 || connectivity > 3 || (class_map && (C != 1 || (applied & 1u)))) return UNETR_ERR_ARG;
    if (C > MORPH_MAXC || !morph_shape_ok(D, H, W) || (long)B * C > MORPH_MAX_PLANES) return UNETR_ERR_UNSUPPORTED;
    const int N = B * C;
    const size_t need = unetr_fill_holes_workspace_bytes(D, H, W, N, class_map);
    if (need > ws_bytes) return UNETR_ERR_WORKSPACE;
    const size_t NV = (size_t)N * D * H * W;
    // the per-root id words first (4-byte aligned at the workspace's start), the per-root face flags behind them
    unsigned* ids = class_map ? (unsigned*)ws : nullptr;
    uint8_t* flag = (uint8_t*)ws + (class_map ? NV * 4 : 0);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, NV * (class_map ? 5 : 1), st) != hipSuccess) return UNETR_ERR_LAUNCH;
    if (u8) return fill_run((const uint8_t*)in, (uint8_t*)out, labels, N, D, H, W, class_map, applied, connectivity, flag, ids, st);
    return fill_run((const float*)in, (float*)out, labels, N, D, H, W, class_map, applied, connectivity, flag, ids, st);
}
