// Hausdorff distance of monai.metrics.HausdorffDistanceMetric (MONAI 0.6.0, euclidean, voxel units) per (b, c), as the
// reference's validation_all_metrics uses it (unetr_segmentation_3d.py:134-209, built at :495-496).  Semantics (DESIGN.md
// section 11): binarise (== 1), crop both masks to the bounding box of pred | gt, drop box axes of extent 1 (np.squeeze),
// edges = m ^ binary_erosion(m) (6-neighbour cross, border 0), distance of every edge voxel of A to the nearest edge voxel
// of B, max or np.percentile, undirected = Python max(d(P->G), d(G->P)).
//
// Launch sequence (one stream, no host sync):
//   hd_bits_kernel      one streaming pass over the inputs: per voxel a class bit word of the prediction and of the ground
//                       truth (argmax / one-hot fused for from_logits), plus z-, y- and x-projections of (pred | gt) by
//                       workgroup-reduced global atomicOr
//   hd_boxes_kernel     per (b, c) union bounding box from the three projections
//   then per group of G (b, c) pairs (workspace slots):
//   hd_xpass_kernel     edges of both masks inside the box (one byte per box voxel) and the 1-D squared distance along x to
//                       the nearest edge of each mask (feature positions of a line compacted in LDS: cost = #features)
//   hd_colpass_kernel   exact min-plus  f(i) = min_j g(j) + (i-j)^2  along y, then along z (32 x-columns per tile, whole
//                       line in LDS, adjacent x in adjacent lanes); the z pass reduces max / count / histogram over the
//                       edges of the other mask instead of storing the transform
//   hd_finalize_kernel  nan / inf rules, sqrt (float64) of the integer maximum or the two order statistics and numpy's lerp
// Squared distances stay integers (< 3 * 512^2) until the final sqrt, so percentile=None results equal scipy's
// distance_transform_edt bit for bit.  "No feature" is HD_INF = 2^30; INF + 511^2 < 2^31, no overflow.
#include <algorithm>
#include <math.h>
#include "common.hpp"
#include "../../include/unetr_hip.h"

namespace {

constexpr int HD_MAXN = 512;          // largest volume extent along every axis (line length of the LDS tiles)
constexpr int HD_MAXC = 32;           // classes in one 32-bit class word
constexpr int HD_INF = 1 << 30;
constexpr int HD_YB = 64;             // rows per workgroup tile of the streaming pass
constexpr int HD_COLS = 32;           // x-columns per tile of the y / z passes
constexpr int HD_NWG = 512;           // workgroups per (b, c) pair in the per-box passes (grid-stride inside)

__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// class word of one voxel: bit c set where the mask of class c is 1
template <bool LOGITS>
__device__ __forceinline__ void class_words(const float* __restrict__ pred, const float* __restrict__ y, int b, int C, long V,
                                            long v, uint32_t& pw, uint32_t& gw) {
    pw = 0u; gw = 0u;
    if (LOGITS) {
        float mx = -3.0e38f;
        int am = 0;
        for (int c = 0; c < C; ++c) {
            const float z = pred[((long)b * C + c) * V + v];
            if (z > mx) { mx = z; am = c; }                 // first maximal channel (torch.argmax, dice_counts_kernel)
        }
        pw = 1u << am;
        const int lab = (int)y[(long)b * V + v];
        gw = (lab >= 0 && lab < C) ? (1u << lab) : 0u;
    } else {
        for (int c = 0; c < C; ++c) {
            if (pred[((long)b * C + c) * V + v] == 1.f) pw |= 1u << c;
            if (y[((long)b * C + c) * V + v] == 1.f) gw |= 1u << c;
        }
    }
}

// grid (ceil(W/64), ceil(H/HD_YB), B*D); wave w of the workgroup takes rows y0 + w, y0 + w + 4, ... of plane z
template <bool LOGITS>
__global__ void __launch_bounds__(256)
hd_bits_kernel(const float* __restrict__ pred, const float* __restrict__ y, int C, int D, int H, int W,
               uint32_t* __restrict__ pbits, uint32_t* __restrict__ gbits, uint32_t* __restrict__ proj) {
    __shared__ uint32_t rows[HD_YB];
    __shared__ uint32_t cols[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.z / D, z = blockIdx.z - b * D;
    const int x = blockIdx.x * 64 + lane, y0 = blockIdx.y * HD_YB;
    const long V = (long)D * H * W;
    uint32_t xacc = 0u;
    for (int r = wave; r < HD_YB; r += 4) {
        const int yy = y0 + r;
        uint32_t u = 0u;
        if (yy < H && x < W) {
            const long v = ((long)z * H + yy) * W + x;
            uint32_t pw, gw;
            class_words<LOGITS>(pred, y, b, C, V, v, pw, gw);
            pbits[(long)b * V + v] = pw;
            gbits[(long)b * V + v] = gw;
            u = pw | gw;
        }
        xacc |= u;
        u = wave_or(u);
        if (lane == 0) rows[r] = u;
    }
    cols[wave][lane] = xacc;
    __syncthreads();
    uint32_t* zp = proj + (long)b * (D + H + W);
    uint32_t* yp = zp + D;
    uint32_t* xp = yp + H;
    if (threadIdx.x < 64) {
        const uint32_t cx = cols[0][lane] | cols[1][lane] | cols[2][lane] | cols[3][lane];
        if (cx && x < W) atomicOr(&xp[x], cx);
        uint32_t rz = 0u;
        for (int r = lane; r < HD_YB; r += 64) {
            const uint32_t ry = rows[r];
            rz |= ry;
            if (ry && y0 + r < H) atomicOr(&yp[y0 + r], ry);
        }
        rz = wave_or(rz);
        if (lane == 0 && rz) atomicOr(&zp[z], rz);
    }
}

// boxes[(b*C + c)*6 ..] = z0, z1, y0, y1, x0, x1 (half-open); an empty union gives all zeros.  One workgroup per b.
__global__ void __launch_bounds__(256)
hd_boxes_kernel(const uint32_t* __restrict__ proj, int C, int D, int H, int W, int* __restrict__ boxes) {
    __shared__ int lo[3][HD_MAXC], hi[3][HD_MAXC];
    const int b = blockIdx.x;
    if (threadIdx.x < 3 * HD_MAXC) {
        (&lo[0][0])[threadIdx.x] = 1 << 30;
        (&hi[0][0])[threadIdx.x] = -1;
    }
    __syncthreads();
    const uint32_t* p = proj + (long)b * (D + H + W);
    for (int i = threadIdx.x; i < D + H + W; i += 256) {
        const int ax = i < D ? 0 : (i < D + H ? 1 : 2);
        const int k = i - (ax == 0 ? 0 : (ax == 1 ? D : D + H));
        uint32_t m = p[i];
        while (m) {
            const int c = __ffs(m) - 1;
            m &= m - 1;
            atomicMin(&lo[ax][c], k);
            atomicMax(&hi[ax][c], k);
        }
    }
    __syncthreads();
    if (threadIdx.x < C) {
        const int c = threadIdx.x;
        int* o = boxes + ((long)b * C + c) * 6;
        const bool any = hi[0][c] >= 0;
        for (int ax = 0; ax < 3; ++ax) {
            o[2 * ax] = any ? lo[ax][c] : 0;
            o[2 * ax + 1] = any ? hi[ax][c] + 1 : 0;
        }
    }
}

struct PairBox {
    int b, c, z0, y0, x0, ez, ey, ex;
};
__device__ __forceinline__ PairBox pair_box(const int* __restrict__ boxes, int C, int c0, int pair) {
    const int Cp = C - c0;
    PairBox p;
    p.b = pair / Cp;
    p.c = c0 + pair % Cp;
    const int* bx = boxes + ((long)p.b * C + p.c) * 6;
    p.z0 = bx[0]; p.y0 = bx[2]; p.x0 = bx[4];
    p.ez = bx[1] - bx[0]; p.ey = bx[3] - bx[2]; p.ex = bx[5] - bx[4];
    return p;
}

// 1 where the voxel is in the mask and has a zero neighbour (an out-of-box neighbour is zero) along some box axis of
// extent > 1 -- m ^ binary_erosion(m) on the squeezed crop
__device__ __forceinline__ int edge_bit(const uint32_t* __restrict__ bits, const PairBox& p, int H, int W, int z, int y, int x) {
    const long v = ((long)(p.z0 + z) * H + (p.y0 + y)) * W + (p.x0 + x);
    const uint32_t m = 1u << p.c;
    if (!(bits[v] & m)) return 0;
    const long HW = (long)H * W;
    if (p.ez > 1 && (z == 0 || z == p.ez - 1 || !(bits[v - HW] & m) || !(bits[v + HW] & m))) return 1;
    if (p.ey > 1 && (y == 0 || y == p.ey - 1 || !(bits[v - W] & m) || !(bits[v + W] & m))) return 1;
    if (p.ex > 1 && (x == 0 || x == p.ex - 1 || !(bits[v - 1] & m) || !(bits[v + 1] & m))) return 1;
    return 0;
}

// grid (HD_NWG, G); every wave takes one x-line (z, y) of the box per iteration (loop trip count uniform per workgroup)
__global__ void __launch_bounds__(256)
hd_xpass_kernel(const uint32_t* __restrict__ pbits, const uint32_t* __restrict__ gbits, const int* __restrict__ boxes,
                int C, int c0, int npairs, int pair0, int D, int H, int W, uint8_t* __restrict__ edges, int* __restrict__ dt,
                long slot_vox) {
    __shared__ int posP[4][HD_MAXN], posG[4][HD_MAXN];
    const int pair = pair0 + blockIdx.y;
    if (pair >= npairs) return;
    const PairBox p = pair_box(boxes, C, c0, pair);
    const long nlines = (long)p.ez * p.ey;
    if (nlines == 0) return;
    const long V = (long)D * H * W;
    const uint32_t* pb = pbits + (long)p.b * V;
    const uint32_t* gb = gbits + (long)p.b * V;
    uint8_t* E = edges + (long)blockIdx.y * slot_vox;
    int* dtP = dt + (long)blockIdx.y * 2 * slot_vox;
    int* dtG = dtP + slot_vox;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long l0 = (long)blockIdx.x * 4; l0 < nlines; l0 += (long)gridDim.x * 4) {
        const long l = l0 + wave;
        const bool valid = l < nlines;
        const int z = valid ? (int)(l / p.ey) : 0, y = valid ? (int)(l - (long)z * p.ey) : 0;
        int nP = 0, nG = 0;
        if (valid) {
            for (int x0 = 0; x0 < p.ex; x0 += 64) {
                const int x = x0 + lane;
                int ep = 0, eg = 0;
                if (x < p.ex) {
                    ep = edge_bit(pb, p, H, W, z, y, x);
                    eg = edge_bit(gb, p, H, W, z, y, x);
                    E[l * p.ex + x] = (uint8_t)(ep | (eg << 1));
                }
                const uint64_t mp = __ballot(ep), mg = __ballot(eg);
                const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
                if (ep) posP[wave][nP + __popcll(mp & below)] = x;
                if (eg) posG[wave][nG + __popcll(mg & below)] = x;
                nP += __popcll(mp);
                nG += __popcll(mg);
            }
        }
        __syncthreads();
        if (valid) {
            for (int x = lane; x < p.ex; x += 64) {
                int fP = HD_INF, fG = HD_INF;
                for (int k = 0; k < nP; ++k) { const int d = x - posP[wave][k]; fP = min(fP, __mul24(d, d)); }
                for (int k = 0; k < nG; ++k) { const int d = x - posG[wave][k]; fG = min(fG, __mul24(d, d)); }
                dtP[l * p.ex + x] = fP;
                dtG[l * p.ex + x] = fG;
            }
        }
        __syncthreads();
    }
}

// grid (HD_NWG, G, 2): blockIdx.z = field (0: distance to the prediction's edges, 1: to the ground truth's edges).
// AXIS 1: lines along y, tiles (z, 32 columns); AXIS 0: lines along z, tiles (y, 32 columns), and the result is reduced
// over the other mask's edges: acc[slot] = {count P, count G, max d2(P->G), max d2(G->P)}, hist[slot][dir][d2].
template <int AXIS>
__global__ void __launch_bounds__(256)
hd_colpass_kernel(const int* __restrict__ boxes, int C, int c0, int npairs, int pair0, int* __restrict__ dt,
                  const uint8_t* __restrict__ edges, long slot_vox, int* __restrict__ acc, int* __restrict__ hist, int nbins) {
    __shared__ int tile[HD_MAXN * HD_COLS];           // 64 KiB; its first 8 words hold the final reduction
    const int pair = pair0 + blockIdx.y;
    if (pair >= npairs) return;
    const PairBox p = pair_box(boxes, C, c0, pair);
    const int field = blockIdx.z;
    const int n = AXIS == 1 ? p.ey : p.ez;             // line length
    const int other = AXIS == 1 ? p.ez : p.ey;
    const int nxc = (p.ex + HD_COLS - 1) / HD_COLS;
    const long ntiles = (long)other * nxc;
    if (ntiles == 0 || n == 0) return;
    int* f = dt + (long)blockIdx.y * 2 * slot_vox + (long)field * slot_vox;
    const uint8_t* E = edges + (long)blockIdx.y * slot_vox;
    const int col = threadIdx.x & (HD_COLS - 1), rg = threadIdx.x / HD_COLS;
    const int qbit = field == 0 ? 2 : 1;               // query set: the OTHER mask's edges
    const int dir = field == 0 ? 1 : 0;                 // 0: P->G (pred edges to gt), 1: G->P
    int lmax = 0, lcnt = 0;
    const long sj = AXIS == 1 ? p.ex : (long)p.ey * p.ex;    // stride between line elements
    for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int o = (int)(t / nxc), x = (int)(t - (long)o * nxc) * HD_COLS + col;
        const long base = (AXIS == 1 ? (long)o * p.ey * p.ex : (long)o * p.ex) + x;
        for (int j = rg; j < n; j += 256 / HD_COLS) tile[j * HD_COLS + col] = x < p.ex ? f[base + j * sj] : HD_INF;
        __syncthreads();
        if (x < p.ex) {
            for (int i = rg; i < n; i += 256 / HD_COLS) {
                int best = HD_INF, d = i * i, step = 1 - 2 * i;   // d = (i - j)^2, advanced by differences
                for (int j = 0; j < n; ++j) {
                    best = min(best, tile[j * HD_COLS + col] + d);
                    d += step;
                    step += 2;
                }
                best = min(best, HD_INF);
                if (AXIS == 1) {
                    f[base + i * sj] = best;
                } else if (E[base + i * sj] & qbit) {
                    lmax = max(lmax, best);
                    ++lcnt;
                    if (hist && best < HD_INF) atomicAdd(&hist[((long)blockIdx.y * 2 + dir) * nbins + best], 1);
                }
            }
        }
        __syncthreads();
    }
    if (AXIS == 0) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        lmax = wave_max_i(lmax);
        lcnt = wave_sum_i(lcnt);
        if (lane == 0) { tile[wave] = lmax; tile[4 + wave] = lcnt; }     // every tile read ended at the loop's barrier
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = max(max(tile[0], tile[1]), max(tile[2], tile[3]));
            const int c = tile[4] + tile[5] + tile[6] + tile[7];
            if (c) {
                atomicAdd(&acc[blockIdx.y * 4 + dir], c);
                atomicMax(&acc[blockIdx.y * 4 + 2 + dir], m);
            }
        }
    }
}

// k-th smallest (0-based) squared distance of direction dir from the histogram; whole workgroup, result in LDS
__device__ int hist_select(const int* __restrict__ h, int nbins, long k, int* sh) {
    __shared__ int found;
    __shared__ long run_sh;
    __syncthreads();                                    // a previous call's readers of found are done
    if (threadIdx.x == 0) { found = -1; run_sh = 0; }
    __syncthreads();
    int res = -1;
    for (int base = 0; base < nbins; base += 256) {
        const int i = base + threadIdx.x;
        const int cnt = i < nbins ? h[i] : 0;
        sh[threadIdx.x] = cnt;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {            // inclusive scan (Hillis-Steele)
            const int a = threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
            __syncthreads();
            sh[threadIdx.x] += a;
            __syncthreads();
        }
        const long run = run_sh;
        const long incl = run + sh[threadIdx.x];
        if (cnt && incl - cnt <= k && k < incl) found = i;
        __syncthreads();
        if (threadIdx.x == 0) run_sh = run + sh[255];
        __syncthreads();
        const int fnd = found;
        if (fnd >= 0) { res = fnd; break; }
    }
    return res;
}

// numpy.lerp as np.percentile(method="linear") applies it, without contraction into fma
__device__ double np_lerp(double a, double b, double t) {
    const double diff = __dsub_rn(b, a);
    if (t >= 0.5) return __dsub_rn(b, __dmul_rn(diff, __dsub_rn(1.0, t)));
    return __dadd_rn(a, __dmul_rn(diff, t));
}

// one workgroup per slot: out[b*(C-c0) + c-c0]
__global__ void __launch_bounds__(256)
hd_finalize_kernel(const int* __restrict__ acc, const int* __restrict__ hist, int nbins, int C, int c0, int npairs, int pair0,
                   int use_pct, double q, int directed, double* __restrict__ out) {
    __shared__ int sh[256];
    const int pair = pair0 + blockIdx.x;
    if (pair >= npairs) return;
    const int* a = acc + blockIdx.x * 4;
    const double nan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
    double d[2];
    for (int dir = 0; dir < (directed ? 1 : 2); ++dir) {
        const long nA = a[dir], nB = a[1 - dir];
        if (nA == 0) { d[dir] = nan; continue; }                 // no query edges: empty distance array
        if (nB == 0) { d[dir] = use_pct ? nan : inf; continue; } // all-inf array: max inf, np.percentile nan
        if (!use_pct) { d[dir] = __dsqrt_rn((double)a[2 + dir]); continue; }
        const double vi = __dmul_rn((double)(nA - 1), q);       // numpy: virtual index (n - 1) * q
        long prev;
        double gamma;
        if (vi >= (double)(nA - 1)) { prev = nA - 1; gamma = __dadd_rn(vi, 1.0); }   // numpy takes index -1 there
        else { prev = (long)floor(vi); gamma = __dsub_rn(vi, (double)prev); }
        const long next = vi >= (double)(nA - 1) ? nA - 1 : prev + 1;
        const int* h = hist + ((long)blockIdx.x * 2 + dir) * nbins;
        const int sp = hist_select(h, nbins, prev, sh);
        const int sn = next == prev ? sp : hist_select(h, nbins, next, sh);
        d[dir] = np_lerp(__dsqrt_rn((double)sp), __dsqrt_rn((double)sn), gamma);
    }
    if (threadIdx.x == 0) {
        double r = d[0];
        if (!directed && d[1] > d[0]) r = d[1];               // Python max(d1, d2): d1 unless d2 > d1
        out[pair] = r;
    }
}

inline size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }

struct HdLayout {
    size_t pbits, gbits, proj, boxes, edges, dt, acc, hist, total, zero_bytes;
    long V;
    int nbins;
};
HdLayout hd_layout(int B, int C, int D, int H, int W, int group, int use_hist) {
    HdLayout L;
    L.V = (long)D * H * W;
    L.nbins = (D - 1) * (D - 1) + (H - 1) * (H - 1) + (W - 1) * (W - 1) + 1;
    size_t o = 0;
    L.pbits = o; o += al256((size_t)B * L.V * 4);
    L.gbits = o; o += al256((size_t)B * L.V * 4);
    L.proj = o; o += al256((size_t)B * (D + H + W) * 4);
    L.boxes = o; o += al256((size_t)B * C * 6 * 4);
    L.edges = o; o += al256((size_t)group * L.V);
    L.dt = o; o += al256((size_t)group * 2 * L.V * 4);
    L.acc = o;                                             // acc and hist are contiguous: one memset per group
    L.hist = L.acc + (size_t)group * 4 * 4;
    L.zero_bytes = (size_t)group * 4 * 4 + (use_hist ? (size_t)group * 2 * L.nbins * 4 : 0);
    o += al256(L.zero_bytes);
    L.total = o;
    return L;
}

}  // namespace

extern "C" size_t unetr_hausdorff_workspace_bytes(int B, int C, int D, int H, int W, int group, int use_percentile) {
    if (B <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0 || group < 0) return 0;
    return hd_layout(B, C, D, H, W, group, use_percentile).total;
}

extern "C" int unetr_hausdorff(const float* pred, const float* y, int B, int C, int D, int H, int W, int c0, int from_logits,
                               int use_percentile, double q, int directed, double* out, void* ws, size_t ws_bytes, int group,
                               void* stream) {
    if (!pred || !y || !out || !ws || B <= 0 || D <= 0 || H <= 0 || W <= 0 || c0 < 0 || c0 >= C || group <= 0) return UNETR_ERR_ARG;
    if (C > HD_MAXC || D > HD_MAXN || H > HD_MAXN || W > HD_MAXN || (long)B * D > 65535) return UNETR_ERR_UNSUPPORTED;
    if (use_percentile && !(q >= 0.0 && q <= 1.0)) return UNETR_ERR_ARG;
    const int npairs = B * (C - c0);
    group = std::min(group, npairs);
    const HdLayout L = hd_layout(B, C, D, H, W, group, use_percentile);
    if (L.total > ws_bytes) return UNETR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    uint32_t* pbits = (uint32_t*)(w + L.pbits);
    uint32_t* gbits = (uint32_t*)(w + L.gbits);
    uint32_t* proj = (uint32_t*)(w + L.proj);
    int* boxes = (int*)(w + L.boxes);
    uint8_t* edges = (uint8_t*)(w + L.edges);
    int* dt = (int*)(w + L.dt);
    int* acc = (int*)(w + L.acc);
    int* hist = use_percentile ? (int*)(w + L.hist) : nullptr;
    if (hipMemsetAsync(proj, 0, (size_t)B * (D + H + W) * 4, st) != hipSuccess) return UNETR_ERR_LAUNCH;
    const dim3 gb(cdiv(W, 64), cdiv(H, HD_YB), B * D);
    if (from_logits) hipLaunchKernelGGL(hd_bits_kernel<true>, gb, dim3(256), 0, st, pred, y, C, D, H, W, pbits, gbits, proj);
    else hipLaunchKernelGGL(hd_bits_kernel<false>, gb, dim3(256), 0, st, pred, y, C, D, H, W, pbits, gbits, proj);
    hipLaunchKernelGGL(hd_boxes_kernel, dim3(B), dim3(256), 0, st, proj, C, D, H, W, boxes);
    for (int pair0 = 0; pair0 < npairs; pair0 += group) {
        if (hipMemsetAsync(acc, 0, L.zero_bytes, st) != hipSuccess) return UNETR_ERR_LAUNCH;
        hipLaunchKernelGGL(hd_xpass_kernel, dim3(HD_NWG, group), dim3(256), 0, st, pbits, gbits, boxes, C, c0, npairs, pair0,
                           D, H, W, edges, dt, L.V);
        hipLaunchKernelGGL(hd_colpass_kernel<1>, dim3(HD_NWG, group, 2), dim3(256), 0, st, boxes, C, c0, npairs, pair0, dt,
                           edges, L.V, acc, hist, L.nbins);
        hipLaunchKernelGGL(hd_colpass_kernel<0>, dim3(HD_NWG, group, 2), dim3(256), 0, st, boxes, C, c0, npairs, pair0, dt,
                           edges, L.V, acc, hist, L.nbins);
        hipLaunchKernelGGL(hd_finalize_kernel, dim3(group), dim3(256), 0, st, acc, hist, L.nbins, C, c0, npairs, pair0,
                           use_percentile, q, directed, out);
        const int rc = unetr_check_launch();
        if (rc) return rc;
    }
    return unetr_check_launch();
}
