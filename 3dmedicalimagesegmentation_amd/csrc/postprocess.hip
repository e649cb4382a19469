// 3-D connected-component labelling and the post-processing built on it (monai.transforms.KeepLargestConnectedComponent,
// MONAI 0.6.0; skimage.morphology.remove_small_objects): DESIGN.md section 15.
//
// A *plane* is one [D, H, W] volume of class words w (one byte per voxel, 0 = not subject to filtering).  Two voxels are
// connected when they are neighbours under the connectivity (1: 6, 2: 18, 3: 26 neighbours) and carry the same non-zero w.
// The label of a component is 1 + the smallest linear index of its voxels, so the result does not depend on thread order.
//
//   init            w(v) from the input, label[v] = start of v's run of equal w within its 64-lane x segment, size[v] = 0
//   merge           label-equivalence union-find over the backward neighbours (atomicMin towards the smaller index)
//   flatten + count label[v] = root(v); size[root] += 1 (integer atomics, runs and whole waves combined first)
//   select          best[plane][w] = max over roots of (size << 32 | ~root); ncomp[plane][w] += 1
//   apply           out = keep ? in : 0, canonical label map, per-voxel component size
//
// One stream-ordered call, fixed grids, no host synchronisation, one workspace: the call can be captured in a graph.
#include "common.hpp"

namespace {

constexpr int CCL_MAXC = 16;      // channels of a one-hot / logits input
constexpr int CCL_WORDS = 32;     // class words 0..31
constexpr int CCL_MAXN = 1024;    // voxels along one axis
constexpr int CCL_BG = -1;        // label of a voxel with w == 0
constexpr int CCL_SEGS = 16;      // 64-voxel segments one wave counts before it issues its atomic
constexpr int CCL_SELECT_BLOCKS = 1024;

struct CclPlan {
    int mode;                     // 0: class-id map [B, 1, V]; 1: one-hot / multi-label [B, C, V]
    int independent;
    unsigned applied;             // mode 0: bit id set = class id filtered
    int nA, chan[CCL_MAXC];       // mode 1: the applied channels
    int C, H, W, V, nseg;         // nseg = 64-lane segments per row
    long S;                       // segments per plane = D * H * nseg
};

__device__ __forceinline__ int ld_rlx(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_rlx(int* p, int x) { __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// class word of voxel v of plane p
__device__ __forceinline__ int ccl_word(const float* __restrict__ in, const CclPlan& P, int p, int v) {
    if (P.mode == 0) {
        const float f = in[(size_t)p * P.V + v];
        if (!(f >= 1.f && f <= 31.f)) return 0;
        const int id = (int)f;
        if (f != (float)id || !((P.applied >> id) & 1u)) return 0;
        return P.independent ? id : 1;
    }
    if (P.independent) {
        const int b = p / P.nA, c = P.chan[p % P.nA];
        return in[((size_t)b * P.C + c) * P.V + v] != 0.f;
    }
    bool any = false;
    for (int k = 0; k < P.nA; ++k) any |= in[((size_t)p * P.C + P.chan[k]) * P.V + v] != 0.f;
    return any;
}

// one wave = one 64-voxel x segment of one row; false past the last segment (wave-uniform)
__device__ __forceinline__ bool ccl_segment(const CclPlan& P, long s, int lane, int& row, int& x, int& v) {
    if (s >= P.S) return false;
    row = (int)(s / P.nseg);
    x = (int)(s % P.nseg) * 64 + lane;
    v = row * P.W + x;
    return true;
}

__global__ __launch_bounds__(256) void ccl_init_kernel(const float* __restrict__ in, CclPlan P, int plane0,
                                                       uint8_t* __restrict__ wb, int* __restrict__ label, int* __restrict__ size) {
    const int lane = threadIdx.x & 63;
    int row, x, v;
    if (!ccl_segment(P, (long)blockIdx.x * 4 + (threadIdx.x >> 6), lane, row, x, v)) return;
    const bool in_row = x < P.W;
    const int w = in_row ? ccl_word(in, P, plane0 + blockIdx.y, v) : 0;
    const int wprev = __shfl_up(w, 1);
    const unsigned long long starts = __ballot(w != 0 && (lane == 0 || wprev != w));
    if (!in_row) return;
    const size_t o = (size_t)blockIdx.y * P.V + v;
    int lab = CCL_BG;
    if (w) {   // the run's first lane: the highest start bit at or below this lane (this lane's own run always has one)
        const unsigned long long m = starts & (~0ull >> (63 - lane));
        lab = v - lane + (63 - __clzll((long long)m));
    }
    wb[o] = (uint8_t)w;
    label[o] = lab;
    size[o] = 0;
}

// Invariant of the label array: label[v] <= v for every foreground voxel, and label[v] only ever decreases (atomicMin).  So a
// chain of parents is strictly decreasing and ends at a root (label[r] == r) after at most v steps -- also when a load returns
// a value another workgroup has since lowered: every value label[v] ever held is a voxel of v's component that is <= v.
__device__ __forceinline__ int ccl_find(const int* L, int v) {
    int p;
    while ((p = ld_rlx(L + v)) != v) v = p;
    return v;
}

__device__ __forceinline__ void ccl_union(int* L, int a, int b) {
    a = ccl_find(L, a);
    b = ccl_find(L, b);
    // Termination: let a be the larger of the pair.  atomicMin returns old <= a.  old == a: a was a root and now points at b,
    // done.  Otherwise the pair becomes (find(old), b) with find(old) <= old < a, so max(a, b) strictly decreases with every
    // retry; it is bounded below by 0, hence the loop ends for any interleaving of workgroups.
    // Correctness: when the atomicMin replaces a's parent old by b, the equivalence a ~ old it stood for is kept by this very
    // thread, which goes on to unite old's root with b; when it leaves old in place (old < b), a ~ b still needs old ~ b,
    // which is again the next pair.  A stale load only picks an older (larger) member of the same component; the atomic, which
    // is performed on the one coherent copy, then returns the current parent and the loop continues from there.
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(L + a, b);
        if (old == a) break;
        a = ccl_find(L, old);
    }
}

template <int CONN>
__global__ __launch_bounds__(256) void ccl_merge_kernel(CclPlan P, const uint8_t* __restrict__ wb, int* label) {
    const int lane = threadIdx.x & 63;
    int row, x, v;
    if (!ccl_segment(P, (long)blockIdx.x * 4 + (threadIdx.x >> 6), lane, row, x, v)) return;
    if (x >= P.W) return;
    const uint8_t* wp = wb + (size_t)blockIdx.y * P.V;
    int* L = label + (size_t)blockIdx.y * P.V;
    const int w = wp[v];
    if (!w) return;
    const int H = P.H, W = P.W;
    const int z = row / H, y = row % H;
    if (lane == 0 && x > 0 && wp[v - 1] == w) ccl_union(L, v, v - 1);        // the run init cut here
    // backward rows (dz, dy) = (-1, -1), (-1, 0), (-1, 1), (0, -1); dx = -1, 0, 1 as far as the connectivity reaches.  Where
    // the centre of a row matches, its two diagonals lie in the centre's run and add nothing.  A union that the x neighbour in
    // v's own run makes with the same run above is left to that neighbour (v ~ v-1 and c ~ c-1 hold through the runs), so
    // inside a solid region only the first voxel of a run unites.
    const bool left = x > 0 && wp[v - 1] == w;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int dz = r < 3 ? -1 : 0, dy = r < 3 ? r - 1 : -1;
        const int m = (dz != 0) + (dy != 0);
        if (m > CONN) continue;
        const int zz = z + dz, yy = y + dy;
        if (zz < 0 || yy < 0 || yy >= H) continue;
        const int c = (zz * H + yy) * W + x;
        if (wp[c] == w) {
            if (!(left && wp[c - 1] == w)) ccl_union(L, v, c);
            continue;
        }
        if (m + 1 > CONN) continue;
        if (!left && x > 0 && wp[c - 1] == w) ccl_union(L, v, c - 1);                  // else v-1 unites with its centre c-1
        if (x + 1 < W && wp[c + 1] == w && wp[v + 1] != w) ccl_union(L, v, c + 1);    // else v+1 unites with its centre c+1
    }
}

// label[v] = root(v) and size[root] += 1.  A wave whose foreground lanes share one root adds its popcount to a carry that
// lives across CCL_SEGS segments; otherwise each run of equal roots along x adds its length once.  The four waves' carries
// are combined through LDS, so one component that fills the volume costs one atomic per 64 * CCL_SEGS * 4 voxels.
__global__ __launch_bounds__(256) void ccl_flatten_count_kernel(CclPlan P, int* label, int* size) {
    __shared__ int s_root[4], s_n[4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int* L = label + (size_t)blockIdx.y * P.V;
    int* sz = size + (size_t)blockIdx.y * P.V;
    const long s0 = ((long)blockIdx.x * 4 + wid) * CCL_SEGS;
    int carry_root = CCL_BG, carry_n = 0;                                    // wave-uniform
    for (int k = 0; k < CCL_SEGS; ++k) {
        int row, x, v;
        if (!ccl_segment(P, s0 + k, lane, row, x, v)) break;
        int root = CCL_BG;
        if (x < P.W) {
            const int p = ld_rlx(L + v);
            if (p != CCL_BG) {
                root = ccl_find(L, p);
                if (root != p) st_rlx(L + v, root);                          // a racing reader sees p or root: both lead to root
            }
        }
        const bool fg = root != CCL_BG;
        const unsigned long long fm = __ballot(fg);
        if (!fm) continue;
        const int first = __shfl(root, __ffsll((long long)fm) - 1);
        if (__ballot(fg && root != first) == 0) {
            if (first != carry_root) {
                if (lane == 0 && carry_n) atomicAdd(sz + carry_root, carry_n);
                carry_root = first;
                carry_n = 0;
            }
            carry_n += __popcll(fm);
            continue;
        }
        if (lane == 0 && carry_n) atomicAdd(sz + carry_root, carry_n);
        carry_root = CCL_BG;
        carry_n = 0;
        const int prev = __shfl_up(root, 1);
        const unsigned long long bounds = __ballot(lane == 0 || prev != root);   // first lanes of runs, background runs included
        if (fg && ((bounds >> lane) & 1)) {
            const unsigned long long next = lane == 63 ? 0ull : bounds & (~0ull << (lane + 1));
            atomicAdd(sz + root, (next ? __ffsll((long long)next) - 1 : 64) - lane);
        }
    }
    if (lane == 0) { s_root[wid] = carry_root; s_n[wid] = carry_n; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 0; i < 4; ++i) {
            int n = s_n[i];
            if (!n) continue;
            for (int j = i + 1; j < 4; ++j)
                if (s_n[j] && s_root[j] == s_root[i]) { n += s_n[j]; s_n[j] = 0; }
            atomicAdd(sz + s_root[i], n);
        }
    }
}

// best[plane][w] = max over the roots of (size << 32 | 0xFFFFFFFF - root): the largest size, ties to the smallest root
__global__ __launch_bounds__(256) void ccl_select_kernel(CclPlan P, const uint8_t* __restrict__ wb, const int* __restrict__ label,
                                                         const int* __restrict__ size, unsigned long long* __restrict__ best,
                                                         int* __restrict__ ncomp) {
    __shared__ unsigned long long s_best[CCL_WORDS];
    __shared__ int s_cnt[CCL_WORDS];
    if (threadIdx.x < CCL_WORDS) { s_best[threadIdx.x] = 0; s_cnt[threadIdx.x] = 0; }
    __syncthreads();
    const size_t base = (size_t)blockIdx.y * P.V;
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < P.V; v += (long)gridDim.x * 256) {
        if (label[base + v] != (int)v) continue;
        const int w = wb[base + v] & (CCL_WORDS - 1);
        atomicMax(&s_best[w], ((unsigned long long)(unsigned)size[base + v] << 32) | (0xFFFFFFFFu - (unsigned)v));
        atomicAdd(&s_cnt[w], 1);
    }
    __syncthreads();
    if (threadIdx.x < CCL_WORDS && s_cnt[threadIdx.x]) {
        atomicMax(best + blockIdx.y * CCL_WORDS + threadIdx.x, s_best[threadIdx.x]);
        atomicAdd(ncomp + blockIdx.y * CCL_WORDS + threadIdx.x, s_cnt[threadIdx.x]);
    }
}

__global__ __launch_bounds__(256) void ccl_apply_kernel(const float* in, float* out, int* __restrict__ lab_out,
                                                        int* __restrict__ size_out, CclPlan P, int plane0, int rule, int min_size,
                                                        const uint8_t* __restrict__ wb, const int* __restrict__ label,
                                                        const int* __restrict__ size, const unsigned long long* __restrict__ best) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= P.V) return;
    const size_t base = (size_t)blockIdx.y * P.V;
    const int p = plane0 + blockIdx.y;
    const int w = wb[base + v];
    int lab = 0, n = 0;
    bool keep = true;
    if (w) {
        const int root = label[base + v];
        lab = root + 1;
        if (rule == 1 || size_out) n = size[base + root];
        keep = rule == 1 ? n >= min_size : (unsigned)best[blockIdx.y * CCL_WORDS + w] == 0xFFFFFFFFu - (unsigned)root;
    }
    if (P.mode == 0 || P.independent) {
        const size_t o = (P.mode == 0 ? (size_t)p : (size_t)(p / P.nA) * P.C + P.chan[p % P.nA]) * P.V + v;
        if (out) out[o] = keep ? in[o] : 0.f;
        if (lab_out) lab_out[o] = lab;
        if (size_out) size_out[o] = n;
        return;
    }
    for (int k = 0; k < P.nA; ++k) {   // one mask for all applied channels of the item
        const size_t o = ((size_t)p * P.C + P.chan[k]) * P.V + v;
        const float f = in[o];
        if (out) out[o] = keep ? f : 0.f;
        if (lab_out) lab_out[o] = f != 0.f ? lab : 0;
        if (size_out) size_out[o] = f != 0.f ? n : 0;
    }
}

// first-maximum argmax over the channels as float class ids (the rule of sw_finalize_post_kernel)
__global__ __launch_bounds__(256) void ccl_argmax_kernel(const float* __restrict__ in, float* __restrict__ ids, int C, long V) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const float* ib = in + (size_t)blockIdx.y * C * V + v;
    float mx = ib[0];
    int am = 0;
    for (int c = 1; c < C; ++c) {
        const float a = ib[(size_t)c * V];
        if (a > mx) { mx = a; am = c; }
    }
    ids[(size_t)blockIdx.y * V + v] = (float)am;
}

struct CclLayout { size_t label, size, w, best, ncomp, zero_bytes, total; };

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

CclLayout ccl_layout(long V, int group) {
    CclLayout L;
    size_t o = 0;
    L.label = o; o += al256((size_t)group * V * 4);
    L.size = o; o += al256((size_t)group * V * 4);
    L.w = o; o += al256((size_t)group * V);
    L.best = o;                                            // best and ncomp are contiguous: one memset per group
    L.ncomp = L.best + (size_t)group * CCL_WORDS * 8;
    L.zero_bytes = (size_t)group * CCL_WORDS * 12;
    o += al256(L.zero_bytes);
    L.total = o;
    return L;
}

bool ccl_shape_ok(int D, int H, int W) {
    return D <= CCL_MAXN && H <= CCL_MAXN && W <= CCL_MAXN && (long)D * H * W < 2147483647L;
}

}  // namespace

extern "C" size_t unetr_ccl_workspace_bytes(int D, int H, int W, int group) {
    if (D <= 0 || H <= 0 || W <= 0 || group < 0 || !ccl_shape_ok(D, H, W)) return 0;
    return ccl_layout((long)D * H * W, group).total;
}

extern "C" int unetr_ccl(const float* in, float* out, int* labels, int* sizes, int* ncomp, int B, int C, int D, int H, int W,
                         int mode, unsigned applied, int independent, int connectivity, int rule, int min_size, void* ws,
                         size_t ws_bytes, int group, void* stream) {
    if (!in || !ws || (!out && !labels && !sizes && !ncomp) || B <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0 || group <= 0)
        return UNETR_ERR_ARG;
    if (mode < 0 || mode > 2 || connectivity < 1 || connectivity > 3 || rule < 0 || rule > 1 || min_size < 0 || !applied)
        return UNETR_ERR_ARG;
    if (C > CCL_MAXC || !ccl_shape_ok(D, H, W)) return UNETR_ERR_UNSUPPORTED;
    if (mode == 0 && (C != 1 || (applied & 1u))) return UNETR_ERR_ARG;
    if (mode == 1 && C < 32 && (applied >> C)) return UNETR_ERR_ARG;
    if (mode == 2 && (C < 2 || !out || (applied & 1u) || (applied >> C))) return UNETR_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const long V = (long)D * H * W;
    CclPlan P = {};
    P.mode = mode == 1;
    P.independent = independent != 0;
    P.applied = applied;
    if (mode == 1)
        for (int c = 0; c < C; ++c)
            if ((applied >> c) & 1u) P.chan[P.nA++] = c;
    P.C = mode == 1 ? C : 1;
    P.H = H; P.W = W; P.V = (int)V;
    P.nseg = cdiv(W, 64);
    P.S = (long)D * H * P.nseg;
    const long planes = mode == 1 && P.independent ? (long)B * P.nA : B;
    if (planes > 2147483647L / CCL_WORDS) return UNETR_ERR_UNSUPPORTED;
    group = (int)std::min<long>(std::min<long>(group, planes), 65535);
    const CclLayout Lo = ccl_layout(V, group);
    if (Lo.total > ws_bytes) return UNETR_ERR_WORKSPACE;
    char* wsb = (char*)ws;
    int* label = (int*)(wsb + Lo.label);
    int* size = (int*)(wsb + Lo.size);
    uint8_t* wb = (uint8_t*)(wsb + Lo.w);
    unsigned long long* best = (unsigned long long*)(wsb + Lo.best);
    int* nc_ws = (int*)(wsb + Lo.ncomp);
    if (mode == 2) {   // logits -> class ids in out, then the class-id route in place
        hipLaunchKernelGGL(ccl_argmax_kernel, dim3(cdiv(V, 256), B), dim3(256), 0, st, in, out, C, V);
        in = out;
    }
    if (ncomp && hipMemsetAsync(ncomp, 0, (size_t)planes * CCL_WORDS * 4, st) != hipSuccess) return UNETR_ERR_LAUNCH;
    const int seg_blocks = cdiv(P.S, 4), count_blocks = cdiv(P.S, 4 * CCL_SEGS);
    const int select_blocks = std::min(cdiv(V, 256), CCL_SELECT_BLOCKS);
    for (long plane0 = 0; plane0 < planes; plane0 += group) {
        const int n = (int)std::min<long>(group, planes - plane0);
        if (hipMemsetAsync(best, 0, Lo.zero_bytes, st) != hipSuccess) return UNETR_ERR_LAUNCH;
        hipLaunchKernelGGL(ccl_init_kernel, dim3(seg_blocks, n), dim3(256), 0, st, in, P, (int)plane0, wb, label, size);
        if (connectivity == 1) hipLaunchKernelGGL(ccl_merge_kernel<1>, dim3(seg_blocks, n), dim3(256), 0, st, P, wb, label);
        else if (connectivity == 2) hipLaunchKernelGGL(ccl_merge_kernel<2>, dim3(seg_blocks, n), dim3(256), 0, st, P, wb, label);
        else hipLaunchKernelGGL(ccl_merge_kernel<3>, dim3(seg_blocks, n), dim3(256), 0, st, P, wb, label);
        hipLaunchKernelGGL(ccl_flatten_count_kernel, dim3(count_blocks, n), dim3(256), 0, st, P, label, size);
        hipLaunchKernelGGL(ccl_select_kernel, dim3(select_blocks, n), dim3(256), 0, st, P, wb, label, size, best,
                           ncomp ? ncomp + plane0 * CCL_WORDS : nc_ws);
        if (out || labels || sizes)
            hipLaunchKernelGGL(ccl_apply_kernel, dim3(cdiv(V, 256), n), dim3(256), 0, st, in, out, labels, sizes, P, (int)plane0,
                               rule, min_size, wb, label, size, best);
        const int rc = unetr_check_launch();
        if (rc) return rc;
    }
    return UNETR_OK;
}
