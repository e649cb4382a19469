// Sparse contingency table of two canonical label maps, and the instance-level metrics that are reductions of it: BraTS-style
// lesion-wise Dice with lesion-level precision / recall / F1, and panoptic quality.
//
// A *plane* is one [D, H, W] volume.  a and b hold, per plane, 0 (not labelled) or a canonical label as unetr_ccl writes it:
// 1 + the linear index of a voxel of the plane.  Labels go up to 2^31, so the table of the pairs (a, b) that share a voxel cannot
// be dense: it is an open-addressing hash table per plane, key (a << 32) | b, 0 = empty slot (both labels are >= 1).
//
//   clear     tables, dense arrays and counters of the group to 0
//   insert    one wave = one 64-voxel x segment of a row, as in postprocess.hip.  Runs of equal (a, b, mask) along x insert once,
//             with the run's length; the same ballots give the per-label voxel counts sizeA[a], sizeB[b] (dense, integer atomics)
//   fold      one thread per slot: a present pair goes into the dense per-label accumulators of its two labels
//   reduce    fixed grid over the dense arrays: integer counts (atomics: exact), and the float64 sum of the per-label terms as one
//             partial per workgroup, every addition in an order that depends on the shapes alone
//   finalize  one workgroup per plane adds the partials in a fixed order and writes the plane's outputs and its overflow flag
//
// One stream-ordered call, fixed grids, no host synchronisation, a workspace sized from the shapes and max_pairs alone: the call
// can be captured in a graph.  No float atomics anywhere: two calls on the same input return the same bits.
#include "common.hpp"

namespace {

typedef unsigned long long u64;

constexpr int LO_MAXN = 1024;             // voxels along one axis (the limit of unetr_ccl, whose labels these are)
constexpr int LO_MAX_PAIRS = 1 << 24;
constexpr int LO_REDUCE_BLOCKS = 1024;    // upper bound of the reduce grid = of the partials per plane
constexpr int LO_CLEAR_BLOCKS = 4096;
constexpr int LO_COUNTERS = 8;           // per plane: pairs, n_a, tp, fn, fp, n_b, tp_b, spare
enum { CNT_PAIRS, CNT_NA, CNT_TP, CNT_FN, CNT_FP, CNT_NB, CNT_TPB };

struct LoPlan {
    int W, V, nseg;                       // nseg = 64-lane segments per row
    long S;                               // segments per plane = D * H * nseg
    unsigned slot_mask;                   // slots - 1
    int mode, min_size, max_pairs, nblk;
};

// the finalizer of MurmurHash3 (public domain): every input bit reaches every output bit
__device__ __forceinline__ u64 lo_hash(u64 k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// counts[slot] += (n, nm) for key, claiming a slot when the key is new.
// Only the value the CAS returns is trusted: it is performed on the one coherent copy of the slot, whereas a plain load may
// return what another XCD's L2 held before the slot was claimed.  A slot goes from 0 to a key once and
// never changes again, so `old` is the slot's final content whenever it is non-zero.
// Termination: the loop visits each of the slots at most once and waits for no other thread -- every iteration is one CAS that
// completes whatever the other workgroups do -- so it ends after at most `slots` steps under any interleaving.  When all slots
// hold other keys the pair is dropped; the pairs counter then stands at `slots` > max_pairs and the plane is flagged.
__device__ __forceinline__ void lo_insert(u64* keys, int* vals, unsigned mask, int* npairs, u64 key, int n, int nm) {
    unsigned s = (unsigned)lo_hash(key) & mask;
    for (unsigned i = 0; i <= mask; ++i, s = (s + 1) & mask) {
        u64 old = atomicCAS(keys + s, 0ull, key);
        if (old == 0ull) {                 // this thread claimed the slot: the one increment of the distinct-pairs counter
            atomicAdd(npairs, 1);
            old = key;
        }
        if (old == key) {
            atomicAdd(vals + 2 * (size_t)s, n);
            if (nm) atomicAdd(vals + 2 * (size_t)s + 1, nm);
            return;
        }
    }
}

// length of the run that starts at `lane`, given the ballot of the first lanes of all runs
__device__ __forceinline__ int lo_run_len(u64 heads, int lane) {
    const u64 next = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
    return (next ? __ffsll((long long)next) - 1 : 64) - lane;
}

// clears the tables, the dense arrays and the counters of a group: a kernel of the call's own, so that the call is kernel nodes
// only when it is captured in a graph
__global__ __launch_bounds__(256) void lo_clear_kernel(u64* __restrict__ p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = 0ull;
}

__global__ __launch_bounds__(256) void lo_insert_kernel(const int* __restrict__ A, const int* __restrict__ B,
                                                        const float* __restrict__ amask, LoPlan P, long plane0, u64* keys, int* vals,
                                                        int* sizeA, int* sizeB, int* counters) {
    const int lane = threadIdx.x & 63;
    const long s = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= P.S) return;                                               // wave-uniform
    const int x = (int)(s % P.nseg) * 64 + lane;
    int a = 0, b = 0, m = 0;
    if (x < P.W) {
        const size_t o = (size_t)(plane0 + blockIdx.y) * P.V + (size_t)(s / P.nseg) * P.W + x;
        a = A[o];
        b = B[o];
        if ((unsigned)(a - 1) >= (unsigned)P.V) a = 0;                  // not a label of this plane: nothing is addressed by it
        if ((unsigned)(b - 1) >= (unsigned)P.V) b = 0;
        m = a && (!amask || amask[o] != 0.f);
    }
    if (!__ballot(a | b)) return;
    const int pa = __shfl_up(a, 1), pb = __shfl_up(b, 1), pm = __shfl_up(m, 1);
    const size_t g = blockIdx.y;
    // voxels per label: a counts under the mask, b always
    const int am = m ? a : 0, pam = pm ? pa : 0;
    const u64 heads_a = __ballot(lane == 0 || am != pam);
    if (am && ((heads_a >> lane) & 1)) atomicAdd(sizeA + g * P.V + (am - 1), lo_run_len(heads_a, lane));
    const u64 heads_b = __ballot(lane == 0 || b != pb);
    if (b && ((heads_b >> lane) & 1)) atomicAdd(sizeB + g * P.V + (b - 1), lo_run_len(heads_b, lane));
    // pairs: a run ends where a, b or the mask changes; lanes where either label is 0 end runs but insert nothing
    const u64 heads = __ballot(lane == 0 || a != pa || b != pb || m != pm);
    if (a && b && ((heads >> lane) & 1)) {
        const int n = lo_run_len(heads, lane);
        lo_insert(keys + g * ((size_t)P.slot_mask + 1), vals + g * 2 * ((size_t)P.slot_mask + 1), P.slot_mask,
                  counters + g * LO_COUNTERS + CNT_PAIRS, ((u64)(unsigned)a << 32) | (unsigned)b, n, m ? n : 0);
    }
}

// mode 0 (lesion-wise): pv[a] += size(b), inter[a] += masked voxels of the pair, bflag[b] |= 1 | (a is not ignored) << 1
// mode 1 (panoptic):    a pair with IoU > 1/2 -- decided in integers -- writes its IoU to iou[a] and sets bflag[b]; a label has at
//                       most one such partner, so each of these words has one writer
__global__ __launch_bounds__(256) void lo_fold_kernel(LoPlan P, const u64* __restrict__ keys, const int* __restrict__ vals,
                                                      const int* __restrict__ sizeA, const int* __restrict__ sizeB, int* pv, int* inter,
                                                      double* iou, int* bflag) {
    const size_t slots = (size_t)P.slot_mask + 1;
    const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= slots) return;
    const size_t g = blockIdx.y;
    const u64 key = keys[g * slots + s];
    if (!key) return;
    // insert stores labels of this plane only; the check keeps every address below inside the workspace whatever a slot holds
    if ((unsigned)(key >> 32) - 1u >= (unsigned)P.V || (unsigned)key - 1u >= (unsigned)P.V) return;
    const size_t ia = g * P.V + ((unsigned)(key >> 32) - 1), ib = g * P.V + ((unsigned)key - 1);
    const int n = vals[2 * (g * slots + s)], nm = vals[2 * (g * slots + s) + 1];
    const int sa = sizeA[ia], sb = sizeB[ib];
    if (P.mode == 0) {
        atomicAdd(pv + ia, sb);
        if (nm) atomicAdd(inter + ia, nm);
        atomicOr(bflag + ib, sa >= P.min_size ? 3 : 1);
    } else {
        const long u = (long)sa + sb - n;
        if (2L * n > u) {
            iou[ia] = (double)n / (double)u;
            bflag[ib] = 1;
        }
    }
}

// sum over the workgroup in a fixed order: xor tree inside each wave, then the four wave sums in order
__device__ __forceinline__ double lo_block_sum(double s, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__device__ __forceinline__ void lo_count(int* dst, int c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(dst, c);
}

__global__ __launch_bounds__(256) void lo_reduce_kernel(LoPlan P, const int* __restrict__ sizeA, const int* __restrict__ sizeB,
                                                        const int* __restrict__ pv, const int* __restrict__ inter,
                                                        const double* __restrict__ iou, const int* __restrict__ bflag, int* counters,
                                                        double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double sh[4];
    const size_t base = (size_t)blockIdx.y * P.V;
    double sum = 0.0;
    int na = 0, tp = 0, fn = 0, fp = 0, nb = 0, tpb = 0;
    for (long l = (long)blockIdx.x * 256 + threadIdx.x; l < P.V; l += (long)gridDim.x * 256) {
        const int sa = sizeA[base + l], sb = sizeB[base + l];
        if (sa > 0) {
            ++na;
            if (P.mode == 0) {
                if (sa >= P.min_size) {
                    const int p = pv[base + l];
                    if (p > 0) { ++tp; sum += (double)(2L * inter[base + l]) / (double)((long)p + sa); }
                    else ++fn;
                }
            } else {
                const double q = iou[base + l];
                if (q > 0.0) { ++tp; sum += q; }
            }
        }
        if (sb > 0) {
            ++nb;
            const int f = bflag[base + l];
            if (!f) ++fp;
            if (f & 2) ++tpb;
        }
    }
    sum = lo_block_sum(sum, sh);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * P.nblk + blockIdx.x] = sum;
    int* c = counters + (size_t)blockIdx.y * LO_COUNTERS;
    lo_count(c + CNT_NA, na);
    lo_count(c + CNT_TP, tp);
    lo_count(c + CNT_FN, fn);
    lo_count(c + CNT_FP, fp);
    lo_count(c + CNT_NB, nb);
    lo_count(c + CNT_TPB, tpb);
}

__global__ __launch_bounds__(256) void lo_finalize_kernel(LoPlan P, long plane0, const int* __restrict__ counters,
                                                          const double* __restrict__ partials, long long* __restrict__ counts,
                                                          double* __restrict__ values) {
#pragma clang fp contract(off)
    __shared__ double sh[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < P.nblk; i += 256) s += partials[(size_t)blockIdx.x * P.nblk + i];
    s = lo_block_sum(s, sh);
    if (threadIdx.x != 0) return;
    const int* c = counters + (size_t)blockIdx.x * LO_COUNTERS;
    const bool over = c[CNT_PAIRS] > P.max_pairs;
    const double nan = __builtin_nan("");
    const long na = c[CNT_NA], nb = c[CNT_NB];
    long tp = c[CNT_TP], fn, fp;
    double v[UNETR_LO_FIELDS] = {};
    if (P.mode == 0) {
        fn = c[CNT_FN]; fp = c[CNT_FP];
        const long tpb = c[CNT_TPB], den = tp + fn + fp;
        const double prec = tpb + fp ? (double)tpb / (double)(tpb + fp) : nan;
        const double rec = tp + fn ? (double)tp / (double)(tp + fn) : nan;
        v[0] = s;
        v[1] = den ? s / (double)den : 1.0;
        v[2] = prec;
        v[3] = rec;
        v[4] = prec != prec || rec != rec ? nan : (prec + rec == 0.0 ? 0.0 : 2.0 * prec * rec / (prec + rec));
    } else {
        fn = na - tp; fp = nb - tp;
        const bool empty = na + nb == 0;
        v[0] = s;
        v[1] = empty ? nan : (tp ? s / (double)tp : 0.0);
        v[2] = empty ? nan : (double)tp / ((double)tp + 0.5 * (double)fp + 0.5 * (double)fn);
        v[3] = v[1] * v[2];
    }
    long long* co = counts + (size_t)(plane0 + blockIdx.x) * UNETR_LO_FIELDS;
    double* vo = values + (size_t)(plane0 + blockIdx.x) * UNETR_LO_FIELDS;
    co[0] = na;
    co[1] = over ? -1 : tp;
    co[2] = over ? -1 : fn;
    co[3] = over ? -1 : fp;
    co[4] = nb;
    co[5] = over ? -1 : (P.mode == 0 ? c[CNT_TPB] : tp);
    co[6] = over;
    co[7] = c[CNT_PAIRS];
    for (int k = 0; k < UNETR_LO_FIELDS; ++k) vo[k] = over && k < 5 ? nan : v[k];
}

struct LoLayout { size_t keys, vals, sizeA, sizeB, acc, bflag, counters, zero_bytes, partials, total; };

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

inline size_t lo_slots(int max_pairs) {
    size_t s = 2;
    while (s < 2 * (size_t)max_pairs) s <<= 1;
    return s;
}

inline int lo_reduce_blocks(long V) { return std::min(cdiv(V, 256), LO_REDUCE_BLOCKS); }

// the tables come first (a caller can read them back), everything up to zero_bytes is cleared once per group
LoLayout lo_layout(long V, size_t slots, int group) {
    LoLayout L;
    size_t o = 0;
    L.keys = o; o += al256((size_t)group * slots * 8);
    L.vals = o; o += al256((size_t)group * slots * 8);
    L.sizeA = o; o += al256((size_t)group * V * 4);
    L.sizeB = o; o += al256((size_t)group * V * 4);
    L.acc = o; o += al256((size_t)group * V * 8);          // mode 0: pv, inter (int32 each); mode 1: iou (float64)
    L.bflag = o; o += al256((size_t)group * V * 4);
    L.counters = o; o += al256((size_t)group * LO_COUNTERS * 4);
    L.zero_bytes = o;
    L.partials = o; o += al256((size_t)group * lo_reduce_blocks(V) * 8);
    L.total = o;
    return L;
}

bool lo_shape_ok(int D, int H, int W, int max_pairs) {
    return D <= LO_MAXN && H <= LO_MAXN && W <= LO_MAXN && (long)D * H * W < 2147483647L && max_pairs <= LO_MAX_PAIRS;
}

}  // namespace

extern "C" size_t unetr_label_overlaps_workspace_bytes(int D, int H, int W, int max_pairs, int group) {
    if (D <= 0 || H <= 0 || W <= 0 || max_pairs < 1 || group < 0 || !lo_shape_ok(D, H, W, max_pairs)) return 0;
    return lo_layout((long)D * H * W, lo_slots(max_pairs), group).total;
}

extern "C" int unetr_label_overlaps(const int* a, const int* b, const float* a_mask, long planes, int D, int H, int W, int mode,
                                    int min_size, int max_pairs, long long* counts, double* values, void* ws, size_t ws_bytes,
                                    int group, void* stream) {
    if (!a || !b || !counts || !values || !ws || planes <= 0 || D <= 0 || H <= 0 || W <= 0 || group <= 0) return UNETR_ERR_ARG;
    if (mode < 0 || mode > 1 || min_size < 0 || max_pairs < 1 || ((uintptr_t)ws & 255)) return UNETR_ERR_ARG;
    if (!lo_shape_ok(D, H, W, max_pairs)) return UNETR_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const long V = (long)D * H * W;
    const size_t slots = lo_slots(max_pairs);
    group = (int)std::min<long>(std::min<long>(group, planes), 65535);
    const LoLayout Lo = lo_layout(V, slots, group);
    if (Lo.total > ws_bytes) return UNETR_ERR_WORKSPACE;
    LoPlan P = {};
    P.W = W; P.V = (int)V;
    P.nseg = cdiv(W, 64);
    P.S = (long)D * H * P.nseg;
    P.slot_mask = (unsigned)(slots - 1);
    P.mode = mode; P.min_size = min_size; P.max_pairs = max_pairs;
    P.nblk = lo_reduce_blocks(V);
    char* wsb = (char*)ws;
    u64* keys = (u64*)(wsb + Lo.keys);
    int* vals = (int*)(wsb + Lo.vals);
    int* sizeA = (int*)(wsb + Lo.sizeA);
    int* sizeB = (int*)(wsb + Lo.sizeB);
    int* pv = (int*)(wsb + Lo.acc);
    int* inter = pv + (size_t)group * V;
    double* iou = (double*)(wsb + Lo.acc);
    int* bflag = (int*)(wsb + Lo.bflag);
    int* counters = (int*)(wsb + Lo.counters);
    double* partials = (double*)(wsb + Lo.partials);
    for (long plane0 = 0; plane0 < planes; plane0 += group) {
        const int n = (int)std::min<long>(group, planes - plane0);
        hipLaunchKernelGGL(lo_clear_kernel, dim3(std::min(cdiv((long)(Lo.zero_bytes / 8), 1024), LO_CLEAR_BLOCKS)), dim3(256), 0, st,
                           (u64*)wsb, Lo.zero_bytes / 8);
        hipLaunchKernelGGL(lo_insert_kernel, dim3(cdiv(P.S, 4), n), dim3(256), 0, st, a, b, a_mask, P, plane0, keys, vals, sizeA, sizeB,
                           counters);
        hipLaunchKernelGGL(lo_fold_kernel, dim3(cdiv((long)slots, 256), n), dim3(256), 0, st, P, keys, vals, sizeA, sizeB, pv, inter, iou,
                           bflag);
        hipLaunchKernelGGL(lo_reduce_kernel, dim3(P.nblk, n), dim3(256), 0, st, P, sizeA, sizeB, pv, inter, iou, bflag, counters,
                           partials);
        hipLaunchKernelGGL(lo_finalize_kernel, dim3(n), dim3(256), 0, st, P, plane0, counters, partials, counts, values);
        const int rc = unetr_check_launch();
        if (rc) return rc;
    }
    return UNETR_OK;
}
