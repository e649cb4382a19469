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
//
// unetr_surface_metrics runs the same front end and the same per-box passes on float64 millimetres (value policy HdF64 instead
// of HdInt: squared distances (s * k)^2, "no edge" = +inf, 16-column tiles) and reduces every surface metric from the one transform: edge count,
// max, sum and count within a per-class tolerance in the z pass, percentiles by a radix select (sm_select_kernel, eight 8-bit
// passes over the 64-bit patterns of the query edges' squared distances, which the z pass leaves in place of the transform),
// sm_finalize_kernel.  DESIGN.md section 11, "Surface metrics in millimetres".
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
constexpr int HD_F64_COLS = 16;       // x-columns per float64 tile: 64 KiB of LDS, two workgroups per CU
constexpr int SM_MAXPCT = 8;          // percentiles per unetr_surface_metrics call
constexpr int SM_TARGETS = 2 * SM_MAXPCT;     // order statistics per direction (two per percentile)
constexpr int SM_PASSES = 8;          // radix select: 8 bits per pass over a 64-bit pattern
constexpr int SM_ACC = 6;             // 64-bit words per slot: count[2], max bits[2], within[2] (index = direction)

// class word of one voxel: bit c set where the mask of class c is 1.  FORM 0: one-hot float channels (== 1), 1: float logits
// and float class ids, 2: uint8 class ids for both (one byte per voxel, never inflated to one-hot)
enum { HD_ONEHOT = 0, HD_LOGITS = 1, HD_IDS = 2 };
template <int FORM>
__device__ __forceinline__ void class_words(const void* __restrict__ pred_, const void* __restrict__ y_, int b, int C, long V,
                                            long v, uint32_t& pw, uint32_t& gw) {
    pw = 0u; gw = 0u;
    if (FORM == HD_IDS) {
        const int pi = ((const uint8_t*)pred_)[(long)b * V + v], gi = ((const uint8_t*)y_)[(long)b * V + v];
        pw = pi < C ? (1u << pi) : 0u;
        gw = gi < C ? (1u << gi) : 0u;
        return;
    }
    const float* __restrict__ pred = (const float*)pred_;
    const float* __restrict__ y = (const float*)y_;
    if (FORM == HD_LOGITS) {
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
template <int FORM>
__global__ void __launch_bounds__(256)
hd_bits_kernel(const void* __restrict__ pred, const void* __restrict__ y, int C, int D, int H, int W,
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
            class_words<FORM>(pred, y, b, C, V, v, pw, gw);
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

// ---- value policies of the per-box passes: what a squared distance is, how one min-plus line is evaluated and what the z pass
// folds over the query edges.  The passes themselves (hd_xpass_kernel, hd_colpass_kernel) are written once.

// integer voxel units (unetr_hausdorff): acc[slot] = {count P, count G, max d2(P->G), max d2(G->P)}, hist[slot][dir][d2]
struct HdInt {
    using T = int;
    static constexpr int COLS = HD_COLS;
    struct Args {
        int* acc;
        int* hist;
        int nbins;
    };
    int lmax, lcnt;
    __device__ static T inf() { return HD_INF; }
    __device__ static T along_x(int k2, const Args&) { return k2; }
    __device__ void begin(const Args&, int, int, const PairBox&, int) { lmax = 0; lcnt = 0; }
    __device__ T min_plus(const T* colp, int i, int n) const {
        int best = HD_INF, d = i * i, step = 1 - 2 * i;          // d = (i - j)^2, advanced by differences
        for (int j = 0; j < n; ++j) {
            best = min(best, colp[j * COLS] + d);
            d += step;
            step += 2;
        }
        return min(best, HD_INF);
    }
    __device__ void visit(T best, T*, const Args& a, int slot, int dir) {
        lmax = max(lmax, best);
        ++lcnt;
        if (a.hist && best < HD_INF) atomicAdd(&a.hist[((long)slot * 2 + dir) * a.nbins + best], 1);
    }
    __device__ void finish(const Args& a, int slot, int dir, void* scratch) {   // every tile read ended at the loop's barrier
        int* red = (int*)scratch;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        lmax = wave_max_i(lmax);
        lcnt = wave_sum_i(lcnt);
        if (lane == 0) { red[wave] = lmax; red[4 + wave] = lcnt; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = max(max(red[0], red[1]), max(red[2], red[3]));
            const int c = red[4] + red[5] + red[6] + red[7];
            if (c) {
                atomicAdd(&a.acc[slot * 4 + dir], c);
                atomicMax(&a.acc[slot * 4 + 2 + dir], m);
            }
        }
    }
};

struct SmTau {
    double v[HD_MAXC];
};

// float64 millimetres (unetr_surface_metrics): acc[slot] = SM_ACC 64-bit words {count, bits of max d2, count d <= tau} x
// direction, partial[slot][dir][workgroup] = this workgroup's sum of d.  Non-negative doubles order as their bit patterns, so
// the maximum is an integer atomicMax; the sum never meets an atomic: every workgroup owns one partial.
struct HdF64 {
    using T = double;
    static constexpr int COLS = HD_F64_COLS;
    struct Args {
        unsigned long long* acc;
        double* partial;
        double s[3];                                         // mm per step along z, y, x
        SmTau tau;                                           // per evaluated class (index c - c0); NaN: nothing is within
    };
    const double* tab;                                       // LDS: tab[k] = (s * k)^2 of this pass's axis
    double lmax, lsum, tau;
    unsigned int lcnt, lwithin;
    __device__ static T inf() { return __longlong_as_double(0x7ff0000000000000ll); }
    __device__ static double sq_mm(double s, int k) {
        const double t = __dmul_rn(s, (double)k);
        return __dmul_rn(t, t);
    }
    // k2 = k * k <= 511^2 is exact in float and so is its root
    __device__ static T along_x(int k2, const Args& a) { return k2 == HD_INF ? inf() : sq_mm(a.s[2], (int)__fsqrt_rn((float)k2)); }
    __device__ void begin(const Args& a, int axis, int n, const PairBox& p, int c0) {   // the first tile's barrier publishes tab
        __shared__ double tab_s[HD_MAXN];
        for (int k = threadIdx.x; k < n; k += 256) tab_s[k] = sq_mm(a.s[axis], k);
        tab = tab_s;
        lmax = 0.0; lsum = 0.0; lcnt = 0u; lwithin = 0u;
        tau = a.tau.v[p.c - c0];
    }
    __device__ T min_plus(const T* colp, int i, int n) const {
        double best = inf();
        for (int j = 0; j < n; ++j) best = fmin(best, __dadd_rn(colp[j * COLS], tab[abs(i - j)]));
        return best;
    }
    __device__ void visit(T best, T* where, const Args&, int, int) {
        *where = best;                                       // the select reads the query edges' d2 from where the z pass lands them
        const double d = __dsqrt_rn(best);
        lmax = fmax(lmax, best);
        lsum = __dadd_rn(lsum, d);
        ++lcnt;
        if (d <= tau) ++lwithin;
    }
    __device__ void finish(const Args& a, int slot, int dir, void* scratch) {
        double* red = (double*)scratch;                      // [0..3] max, [4..7] sum, then 8 counters
        unsigned int* redc = (unsigned int*)(red + 8);
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {                   // a fixed tree: the sum is reproducible
            lmax = fmax(lmax, __shfl_xor(lmax, o, 64));
            lsum = __dadd_rn(lsum, __shfl_xor(lsum, o, 64));
        }
        lcnt = wave_sum_u(lcnt);
        lwithin = wave_sum_u(lwithin);
        if (lane == 0) { red[wave] = lmax; red[4 + wave] = lsum; redc[wave] = lcnt; redc[4 + wave] = lwithin; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned int c = redc[0] + redc[1] + redc[2] + redc[3];
            if (c) {
                unsigned long long* acc = a.acc + (long)slot * SM_ACC;
                atomicAdd(&acc[dir], (unsigned long long)c);
                atomicMax(&acc[2 + dir], (unsigned long long)__double_as_longlong(fmax(fmax(red[0], red[1]), fmax(red[2], red[3]))));
                atomicAdd(&acc[4 + dir], (unsigned long long)(redc[4] + redc[5] + redc[6] + redc[7]));
                a.partial[((long)slot * 2 + dir) * HD_NWG + blockIdx.x] =
                    __dadd_rn(__dadd_rn(red[4], red[5]), __dadd_rn(red[6], red[7]));
            }
        }
    }
};

// grid (HD_NWG, G); every wave takes one x-line (z, y) of the box per iteration (loop trip count uniform per workgroup)
template <class M>
__global__ void __launch_bounds__(256)
hd_xpass_kernel(const uint32_t* __restrict__ pbits, const uint32_t* __restrict__ gbits, const int* __restrict__ boxes,
                int C, int c0, int npairs, int pair0, int D, int H, int W, uint8_t* __restrict__ edges,
                typename M::T* __restrict__ dt, long slot_vox, typename M::Args a) {
    using T = typename M::T;
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
    T* dtP = dt + (long)blockIdx.y * 2 * slot_vox;
    T* dtG = dtP + slot_vox;
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
                int fP = HD_INF, fG = HD_INF;                  // squared steps to the nearest edge along the line
                for (int k = 0; k < nP; ++k) { const int d = x - posP[wave][k]; fP = min(fP, __mul24(d, d)); }
                for (int k = 0; k < nG; ++k) { const int d = x - posG[wave][k]; fG = min(fG, __mul24(d, d)); }
                dtP[l * p.ex + x] = M::along_x(fP, a);
                dtG[l * p.ex + x] = M::along_x(fG, a);
            }
        }
        __syncthreads();
    }
}

// grid (HD_NWG, G, 2): blockIdx.z = field (0: distance to the prediction's edges, 1: to the ground truth's edges).
// AXIS 1: lines along y, tiles (z, COLS columns); AXIS 0: lines along z, tiles (y, COLS columns), and the result is reduced
// over the other mask's edges by the policy (visit / finish) instead of being stored.
template <int AXIS, class M>
__global__ void __launch_bounds__(256)
hd_colpass_kernel(const int* __restrict__ boxes, int C, int c0, int npairs, int pair0, typename M::T* __restrict__ dt,
                  const uint8_t* __restrict__ edges, long slot_vox, typename M::Args a) {
    using T = typename M::T;
    constexpr int COLS = M::COLS, ROWS = 256 / COLS;
    __shared__ T tile[HD_MAXN * COLS];                // 64 KiB; its first words hold the final reduction
    const int pair = pair0 + blockIdx.y;
    if (pair >= npairs) return;
    const PairBox p = pair_box(boxes, C, c0, pair);
    const int field = blockIdx.z;
    const int n = AXIS == 1 ? p.ey : p.ez;             // line length
    const int other = AXIS == 1 ? p.ez : p.ey;
    const int nxc = (p.ex + COLS - 1) / COLS;
    const long ntiles = (long)other * nxc;
    if (ntiles == 0 || n == 0) return;
    T* f = dt + (long)blockIdx.y * 2 * slot_vox + (long)field * slot_vox;
    const uint8_t* E = edges + (long)blockIdx.y * slot_vox;
    const int col = threadIdx.x & (COLS - 1), rg = threadIdx.x / COLS;
    const int qbit = field == 0 ? 2 : 1;               // query set: the OTHER mask's edges
    const int dir = field == 0 ? 1 : 0;                 // 0: P->G (pred edges to gt), 1: G->P
    M m;
    m.begin(a, AXIS, n, p, c0);
    const long sj = AXIS == 1 ? p.ex : (long)p.ey * p.ex;    // stride between line elements
    for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int o = (int)(t / nxc), x = (int)(t - (long)o * nxc) * COLS + col;
        const long base = (AXIS == 1 ? (long)o * p.ey * p.ex : (long)o * p.ex) + x;
        for (int j = rg; j < n; j += ROWS) tile[j * COLS + col] = x < p.ex ? f[base + j * sj] : M::inf();
        __syncthreads();
        if (x < p.ex) {
            for (int i = rg; i < n; i += ROWS) {
                const T best = m.min_plus(tile + col, i, n);
                if (AXIS == 1) f[base + i * sj] = best;
                else if (E[base + i * sj] & qbit) m.visit(best, &f[base + i * sj], a, blockIdx.y, dir);
            }
        }
        __syncthreads();
    }
    if (AXIS == 0) m.finish(a, blockIdx.y, dir, tile);
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

// the two order statistics (0-based ranks) and the weight np.percentile's linear rule takes of nA ascending values
__device__ __forceinline__ void pct_ranks(long nA, double q, long& prev, long& next, double& gamma) {
    const double vi = __dmul_rn((double)(nA - 1), q);           // numpy: virtual index (n - 1) * q
    if (vi >= (double)(nA - 1)) { prev = nA - 1; gamma = __dadd_rn(vi, 1.0); }   // numpy takes index -1 there
    else { prev = (long)floor(vi); gamma = __dsub_rn(vi, (double)prev); }
    next = vi >= (double)(nA - 1) ? nA - 1 : prev + 1;
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
        long prev, next;
        double gamma;
        pct_ranks(nA, q, prev, next, gamma);
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

// ---- percentiles of the float64 path: radix select over the bit patterns of the query edges' squared distances

struct SmPct {
    double q[SM_MAXPCT];                                     // fractions in [0, 1]
    int n;
};

// target t of a direction = order statistic t & 1 (prev / next) of percentile t >> 1; state[slot][dir][t] = {the leading bits
// of its pattern found so far, its rank among the values that share them}.

// grid (HD_NWG, G, 2): blockIdx.z = direction.  Pass `pass` counts, per target, the next 8 bits of every query edge's d2 whose
// leading 8 * pass bits equal the target's prefix.  A direction with an empty edge set on either side has no percentile to
// find and exits; in every other direction both sets are non-empty, so every stored d2 is finite (no +inf patterns).
__global__ void __launch_bounds__(256)
sm_select_kernel(const int* __restrict__ boxes, int C, int c0, int npairs, int pair0, const double* __restrict__ dt,
                 const uint8_t* __restrict__ edges, long slot_vox, const unsigned long long* __restrict__ acc,
                 const unsigned long long* __restrict__ state, unsigned int* __restrict__ sel, int T, int pass) {
    __shared__ unsigned int h[SM_TARGETS * 256];
    __shared__ unsigned long long prefix[SM_TARGETS];
    const int pair = pair0 + blockIdx.y;
    if (pair >= npairs) return;
    const int dir = blockIdx.z;
    const unsigned long long* a = acc + (long)blockIdx.y * SM_ACC;
    if (a[dir] == 0 || a[1 - dir] == 0) return;
    const PairBox p = pair_box(boxes, C, c0, pair);
    const long nvox = (long)p.ez * p.ey * p.ex;
    const long sd = (long)blockIdx.y * 2 + dir;
    if ((int)threadIdx.x < T) prefix[threadIdx.x] = pass == 0 ? 0ull : state[(sd * SM_TARGETS + threadIdx.x) * 2];
    for (int i = threadIdx.x; i < SM_TARGETS * 256; i += 256) h[i] = 0u;
    __syncthreads();
    const double* f = dt + (long)blockIdx.y * 2 * slot_vox + (long)(1 - dir) * slot_vox;   // P->G reads the field of G's edges
    const uint8_t* E = edges + (long)blockIdx.y * slot_vox;
    const int qbit = dir == 0 ? 1 : 2;
    const int shift = 56 - 8 * pass;
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nvox; v += (long)gridDim.x * 256) {
        if (!(E[v] & qbit)) continue;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(f[v]);
        const unsigned long long lead = pass == 0 ? 0ull : bits >> (shift + 8);
        const unsigned int digit = (unsigned int)(bits >> shift) & 255u;
        for (int t = 0; t < T; ++t)
            if (lead == prefix[t]) atomicAdd(&h[t * 256 + digit], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < T * 256; i += 256)
        if (h[i]) atomicAdd(&sel[sd * SM_TARGETS * 256 + i], h[i]);
}

// grid (G, 2): after select pass `pass`, every target picks the digit its rank falls into (one wave per target: 4 bins per
// lane, a wave scan), appends it to its prefix and leaves the histogram zeroed for the next pass.
__global__ void __launch_bounds__(256)
sm_refine_kernel(int npairs, int pair0, const unsigned long long* __restrict__ acc, unsigned long long* __restrict__ state,
                 unsigned int* __restrict__ sel, SmPct pct, int pass) {
    if (pair0 + (int)blockIdx.x >= npairs) return;
    const int dir = blockIdx.y;
    const unsigned long long* a = acc + (long)blockIdx.x * SM_ACC;
    const long nA = (long)a[dir];
    if (nA == 0 || a[1 - dir] == 0) return;
    const long sd = (long)blockIdx.x * 2 + dir;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = wave; t < 2 * pct.n; t += 4) {
        unsigned long long* stt = state + (sd * SM_TARGETS + t) * 2;
        unsigned long long prefix = 0ull;
        long rank;
        if (pass == 0) {
            long prev, next;
            double gamma;
            pct_ranks(nA, pct.q[t >> 1], prev, next, gamma);
            rank = (t & 1) ? next : prev;
        } else {
            prefix = stt[0];
            rank = (long)stt[1];
        }
        unsigned int* h = sel + (sd * SM_TARGETS + t) * 256 + 4 * lane;
        const long c[4] = {(long)h[0], (long)h[1], (long)h[2], (long)h[3]};
        h[0] = 0u; h[1] = 0u; h[2] = 0u; h[3] = 0u;
        const long s = c[0] + c[1] + c[2] + c[3];
        long incl = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        long below = incl - s;
        const uint64_t hit = __ballot(s > 0 && rank >= below && rank < incl);
        const int src = hit ? __ffsll((unsigned long long)hit) - 1 : 63;       // the rank is below the total: one lane holds it
        int digit = 4 * lane + 3;
        for (int k = 0; k < 3; ++k) {
            if (rank < below + c[k]) { digit = 4 * lane + k; break; }
            below += c[k];
        }
        digit = __shfl(digit, src, 64);
        below = __shfl(below, src, 64);
        if (lane == 0) {
            stt[0] = (prefix << 8) | (unsigned long long)digit;
            stt[1] = (unsigned long long)(rank - below);
        }
    }
}

// out is [8 + 2 * npct][npairs]: n_pred, n_gt, max P->G, max G->P, mean P->G, mean G->P, within P->G, within G->P, then the
// percentiles P->G and the percentiles G->P.  One workgroup per slot.
__global__ void __launch_bounds__(256)
sm_finalize_kernel(const unsigned long long* __restrict__ acc, const double* __restrict__ partial,
                   const unsigned long long* __restrict__ state, int npairs, int pair0, SmPct pct, double* __restrict__ out) {
    __shared__ double sum_s[2][256];
    __shared__ double stat[2][SM_TARGETS];
    const int pair = pair0 + blockIdx.x;
    if (pair >= npairs) return;
    const unsigned long long* a = acc + (long)blockIdx.x * SM_ACC;
    const double nan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
    for (int dir = 0; dir < 2; ++dir) {                        // the workgroups' partial sums, always in the same order
        const double* ps = partial + ((long)blockIdx.x * 2 + dir) * HD_NWG;
        double s = 0.0;
        for (int i = threadIdx.x; i < HD_NWG; i += 256) s = __dadd_rn(s, ps[i]);
        sum_s[dir][threadIdx.x] = s;
    }
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sum_s[0][threadIdx.x] = __dadd_rn(sum_s[0][threadIdx.x], sum_s[0][threadIdx.x + o]);
            sum_s[1][threadIdx.x] = __dadd_rn(sum_s[1][threadIdx.x], sum_s[1][threadIdx.x + o]);
        }
        __syncthreads();
    }
    const int T = 2 * pct.n;
    if ((int)threadIdx.x < 2 * T) {
        const int dir = threadIdx.x / T, t = threadIdx.x - dir * T;
        const long nA = (long)a[dir], nB = (long)a[1 - dir];
        if (nA && nB)       // after the last pass the prefix is the whole pattern
            stat[dir][t] = __dsqrt_rn(__longlong_as_double((long long)state[(((long)blockIdx.x * 2 + dir) * SM_TARGETS + t) * 2]));
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int dir = threadIdx.x;
        const long nA = (long)a[dir], nB = (long)a[1 - dir];
        double* o = out + pair;
        o[(long)dir * npairs] = (double)nA;
        // no query edges: an empty distance array (nan everywhere).  No edges to measure to: an all-inf array, whose max and
        // mean are inf and whose np.percentile is nan.
        o[(long)(2 + dir) * npairs] = nA == 0 ? nan : (nB == 0 ? inf : __dsqrt_rn(__longlong_as_double((long long)a[2 + dir])));
        o[(long)(4 + dir) * npairs] = nA == 0 ? nan : (nB == 0 ? inf : __ddiv_rn(sum_s[dir][0], (double)nA));
        o[(long)(6 + dir) * npairs] = (double)a[4 + dir];
        for (int k = 0; k < pct.n; ++k) {
            double r = nan;
            if (nA && nB) {
                long prev, next;
                double gamma;
                pct_ranks(nA, pct.q[k], prev, next, gamma);
                r = np_lerp(stat[dir][2 * k], stat[dir][2 * k + 1], gamma);
            }
            o[(long)(8 + dir * pct.n + k) * npairs] = r;
        }
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

// unetr_surface_metrics: the same front, 16 B of transform per slot voxel, then acc | partial | state | sel, zeroed together
// per group
struct SmLayout {
    size_t pbits, gbits, proj, boxes, edges, dt, acc, partial, state, sel, total, zero_bytes;
    long V;
};
SmLayout sm_layout(int B, int C, int D, int H, int W, int group, int npct) {
    SmLayout L;
    L.V = (long)D * H * W;
    size_t o = 0;
    L.pbits = o; o += al256((size_t)B * L.V * 4);
    L.gbits = o; o += al256((size_t)B * L.V * 4);
    L.proj = o; o += al256((size_t)B * (D + H + W) * 4);
    L.boxes = o; o += al256((size_t)B * C * 6 * 4);
    L.edges = o; o += al256((size_t)group * L.V);
    L.dt = o; o += al256((size_t)group * 2 * L.V * 8);
    L.acc = o;
    L.partial = L.acc + (size_t)group * SM_ACC * 8;
    L.state = L.partial + (size_t)group * 2 * HD_NWG * 8;
    L.sel = L.state + (size_t)group * 2 * SM_TARGETS * 2 * 8;
    L.zero_bytes = (L.sel - L.acc) + (npct ? (size_t)group * 2 * SM_TARGETS * 256 * 4 : 0);
    o += al256(L.zero_bytes);
    L.total = o;
    return L;
}

// class words and union boxes of the whole batch (shared by both entry points)
int hd_front(const void* pred, const void* y, int form, int B, int C, int D, int H, int W, uint32_t* pbits, uint32_t* gbits,
             uint32_t* proj, int* boxes, hipStream_t st) {
    if (hipMemsetAsync(proj, 0, (size_t)B * (D + H + W) * 4, st) != hipSuccess) return UNETR_ERR_LAUNCH;
    const dim3 gb(cdiv(W, 64), cdiv(H, HD_YB), B * D);
    if (form == HD_LOGITS) hipLaunchKernelGGL(hd_bits_kernel<HD_LOGITS>, gb, dim3(256), 0, st, pred, y, C, D, H, W, pbits, gbits, proj);
    else if (form == HD_IDS) hipLaunchKernelGGL(hd_bits_kernel<HD_IDS>, gb, dim3(256), 0, st, pred, y, C, D, H, W, pbits, gbits, proj);
    else hipLaunchKernelGGL(hd_bits_kernel<HD_ONEHOT>, gb, dim3(256), 0, st, pred, y, C, D, H, W, pbits, gbits, proj);
    hipLaunchKernelGGL(hd_boxes_kernel, dim3(B), dim3(256), 0, st, proj, C, D, H, W, boxes);
    return 0;
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
    int* boxes = (int*)(w + L.boxes);
    uint8_t* edges = (uint8_t*)(w + L.edges);
    int* dt = (int*)(w + L.dt);
    HdInt::Args a;
    a.acc = (int*)(w + L.acc);
    a.hist = use_percentile ? (int*)(w + L.hist) : nullptr;
    a.nbins = L.nbins;
    const int frc = hd_front(pred, y, from_logits ? HD_LOGITS : HD_ONEHOT, B, C, D, H, W, pbits, gbits, (uint32_t*)(w + L.proj),
                             boxes, st);
    if (frc) return frc;
    for (int pair0 = 0; pair0 < npairs; pair0 += group) {
        if (hipMemsetAsync(a.acc, 0, L.zero_bytes, st) != hipSuccess) return UNETR_ERR_LAUNCH;
        hipLaunchKernelGGL(hd_xpass_kernel<HdInt>, dim3(HD_NWG, group), dim3(256), 0, st, pbits, gbits, boxes, C, c0, npairs,
                           pair0, D, H, W, edges, dt, L.V, a);
        hipLaunchKernelGGL((hd_colpass_kernel<1, HdInt>), dim3(HD_NWG, group, 2), dim3(256), 0, st, boxes, C, c0, npairs, pair0,
                           dt, edges, L.V, a);
        hipLaunchKernelGGL((hd_colpass_kernel<0, HdInt>), dim3(HD_NWG, group, 2), dim3(256), 0, st, boxes, C, c0, npairs, pair0,
                           dt, edges, L.V, a);
        hipLaunchKernelGGL(hd_finalize_kernel, dim3(group), dim3(256), 0, st, a.acc, a.hist, L.nbins, C, c0, npairs, pair0,
                           use_percentile, q, directed, out);
        const int rc = unetr_check_launch();
        if (rc) return rc;
    }
    return unetr_check_launch();
}

extern "C" size_t unetr_surface_metrics_workspace_bytes(int B, int C, int D, int H, int W, int group, int npct) {
    if (B <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0 || group < 0 || npct < 0) return 0;
    return sm_layout(B, C, D, H, W, group, npct).total;
}

extern "C" int unetr_surface_metrics(const void* pred, const void* y, int B, int C, int D, int H, int W, int c0, int input_form,
                                     const double* spacing, const double* percentiles, int npct, const double* thresholds,
                                     double* out, void* ws, size_t ws_bytes, int group, void* stream) {
    if (!pred || !y || !out || !ws || !spacing || B <= 0 || D <= 0 || H <= 0 || W <= 0 || c0 < 0 || c0 >= C || group <= 0)
        return UNETR_ERR_ARG;
    if (input_form < HD_ONEHOT || input_form > HD_IDS || npct < 0 || (npct > 0 && !percentiles)) return UNETR_ERR_ARG;
    if (C > HD_MAXC || D > HD_MAXN || H > HD_MAXN || W > HD_MAXN || (long)B * D > 65535 || npct > SM_MAXPCT)
        return UNETR_ERR_UNSUPPORTED;
    HdF64::Args a;
    SmPct pct;
    for (int k = 0; k < 3; ++k) {
        if (!(spacing[k] > 0.0) || !std::isfinite(spacing[k])) return UNETR_ERR_ARG;
        a.s[k] = spacing[k];
    }
    for (int k = 0; k < SM_MAXPCT; ++k) {
        pct.q[k] = k < npct ? percentiles[k] : 0.0;
        if (!(pct.q[k] >= 0.0 && pct.q[k] <= 1.0)) return UNETR_ERR_ARG;
    }
    pct.n = npct;
    for (int c = 0; c < HD_MAXC; ++c) a.tau.v[c] = (thresholds && c < C - c0) ? thresholds[c] : (double)NAN;
    const int npairs = B * (C - c0);
    group = std::min(group, npairs);
    const SmLayout L = sm_layout(B, C, D, H, W, group, npct);
    if (L.total > ws_bytes) return UNETR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    uint32_t* pbits = (uint32_t*)(w + L.pbits);
    uint32_t* gbits = (uint32_t*)(w + L.gbits);
    int* boxes = (int*)(w + L.boxes);
    uint8_t* edges = (uint8_t*)(w + L.edges);
    double* dt = (double*)(w + L.dt);
    unsigned int* sel = (unsigned int*)(w + L.sel);
    unsigned long long* state = (unsigned long long*)(w + L.state);
    a.acc = (unsigned long long*)(w + L.acc);
    a.partial = (double*)(w + L.partial);
    const int frc = hd_front(pred, y, input_form, B, C, D, H, W, pbits, gbits, (uint32_t*)(w + L.proj), boxes, st);
    if (frc) return frc;
    for (int pair0 = 0; pair0 < npairs; pair0 += group) {
        if (hipMemsetAsync(a.acc, 0, L.zero_bytes, st) != hipSuccess) return UNETR_ERR_LAUNCH;
        hipLaunchKernelGGL(hd_xpass_kernel<HdF64>, dim3(HD_NWG, group), dim3(256), 0, st, pbits, gbits, boxes, C, c0, npairs,
                           pair0, D, H, W, edges, dt, L.V, a);
        hipLaunchKernelGGL((hd_colpass_kernel<1, HdF64>), dim3(HD_NWG, group, 2), dim3(256), 0, st, boxes, C, c0, npairs, pair0,
                           dt, edges, L.V, a);
        hipLaunchKernelGGL((hd_colpass_kernel<0, HdF64>), dim3(HD_NWG, group, 2), dim3(256), 0, st, boxes, C, c0, npairs, pair0,
                           dt, edges, L.V, a);
        for (int pass = 0; pass < (npct ? SM_PASSES : 0); ++pass) {
            hipLaunchKernelGGL(sm_select_kernel, dim3(HD_NWG, group, 2), dim3(256), 0, st, boxes, C, c0, npairs, pair0, dt, edges,
                               L.V, a.acc, state, sel, 2 * npct, pass);
            hipLaunchKernelGGL(sm_refine_kernel, dim3(group, 2), dim3(256), 0, st, npairs, pair0, a.acc, state, sel, pct, pass);
        }
        hipLaunchKernelGGL(sm_finalize_kernel, dim3(group), dim3(256), 0, st, a.acc, a.partial, state, npairs, pair0, pct, out);
        const int rc = unetr_check_launch();
        if (rc) return rc;
    }
    return unetr_check_launch();
}
