/*
 * unetr_hip.h -- C ABI of libunetr_hip.so, the MI355X (gfx950) kernels behind UNETR's training hot path.
 *
 * The reference (ilkyyldz95/3DmedicalImageSegmentation) has no native code and no FFI: its hot path is
 * `UNETR(nn.Module)` (unetr.py:21-208) delegating to MONAI 0.6.0 blocks and torch ATen ops.  The boundary
 * a maintainer binds is therefore the nn.Module; this header is the C-ABI layer that
 * module calls through ctypes.  Each entry point cites the reference call it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 data unless stated; nothing is allocated or freed here;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no host synchronisation;
 *   - return value 0 = ok, non-zero = UNETR_ERR_* (the Python shim raises RuntimeError);
 *   - `prec`: 0 = fp32 (v_mfma_f32_16x16x4_f32, bit-exact fp32 fma chains), 1 = bf16 operands with fp32
 *     accumulation (v_mfma_f32_16x16x32_bf16), 2 = "bf16x3": fp32 storage like prec 0, every operand element split into a
 *     bf16 (hi, lo) pair inside the kernels and contracted with two bf16 MFMAs per chunk pair (hi*hi + hi*lo + lo*hi + lo*lo,
 *     fp32 accumulation): ~16-bit products at four times the fp32 matrix rate -- the tolerance-grade mode (1e-3 on logits);
 *   - ACTIVATION STORAGE: on the conv side (3x3x3 / 1x1x1 / transposed convs, InstanceNorm, concat copies, out conv)
 *     every feature map and feature-map gradient is stored in the precision mode's activation type: fp32 with prec 0,
 *     **bf16 with prec 1** (half the HBM bytes of passes that are bandwidth-bound; statistics, weights, partial sums,
 *     logits and the input image stay fp32).  Entry points that take `prec` infer the type from it (`const void*`
 *     operands); entry points without one take `act16` (1 = bf16 feature maps).  Rows of a bf16 feature map are 16-byte
 *     aligned (pitch % 8 == 0).  The token side (ViT) keeps an fp32 residual stream plus bf16 operand copies;
 *   - feature maps are channels-last: [B, D, H, W, C] with a row pitch `ld` (floats between voxels), so a
 *     producer can write straight into one half of a concatenation buffer (torch.cat at MONAI
 *     UnetrUpBlock.forward, used by unetr.py:203-206, becomes free);
 *   - token matrices are [B*L, H] row-major, which IS the channels-last view of unetr.py:177-180 proj_feat.
 */
#ifndef UNETR_HIP_H
#define UNETR_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an exported signature or a descriptor struct changes.  A binding (3dmedicalimagesegmentation_amd/_capi.py, or a
 * C caller) must compare unetr_abi_version() with the UNETR_ABI_VERSION it was written against before its first call: a stale
 * .so would otherwise shift arguments silently (a stream pointer in an int slot). */
#define UNETR_ABI_VERSION 21
int unetr_abi_version(void);

/* ---- generic MFMA GEMM: C[M,N] = epilogue(A[M,K] * B[K,N]) ------------------------------------------
 * replaces torch.nn.Linear forward/backward inside MONAI ViT (PatchEmbeddingBlock Linear, SABlock.qkv,
 * SABlock.out_proj, MLPBlock.linear1/2 -- built at unetr.py:78-89) and the 1x1x1 Conv3d of UnetResBlock.conv3
 * (unetr.py:90-174).  a_trans=0: A[m*lda+k]; a_trans=1: A[k*lda+m].  b_trans=0: B[n*ldb+k] (a torch
 * Linear weight [N,K]); b_trans=1: B[k*ldb+n]. */
typedef struct {
    int M, N, K, batch;
    int a_trans, b_trans;
    long lda, ldb, ldc;
    long strideA, strideB, strideC;   /* per-batch element strides */
    const float* bias;                /* [N] or NULL */
    const float* res;                 /* residual added after activation, row index = m % res_mod */
    long ldr, strideR;
    int res_mod;
    float* pre;                       /* optional copy of the pre-activation value (same ld as C) */
    const float* aux;                 /* act==2: multiply by gelu'(aux[m*ldaux+n]) */
    long ldaux;
    int act;                          /* 0 none, 1 exact-erf GELU, 2 GELU backward */
    int accumulate;                   /* C += result */
    float alpha;
    int prec;
    int b_x3words;                    /* prec == UNETR_PREC_BF16X3 only: B holds pre-split words [hi | lo << 16] (unetr_split_words of the
                                       * fp32 weight, same layout and pitch) instead of fp32 values -- the optimizer-maintained word shadow */
} unetr_gemm_desc;
int unetr_gemm(const unetr_gemm_desc* d, const float* A, const float* B, float* C,
               float* ws, size_t ws_bytes, void* stream);
/* bf16x3 mode: dst[i] = [hi | lo << 16] with hi = src[i] truncated to bf16, lo = bf16(src[i] - hi) (n % 4 == 0, 16-byte aligned):
 * the word shadow of a weight arena, re-derived after every optimizer step, that unetr_gemm reads with b_x3words = 1 */
int unetr_split_words(const float* src, void* dst, long n, void* stream);

/* ---- bf16-STORED operand GEMM (LDS-DMA staged): the same nn.Linear forward / data-gradient calls as unetr_gemm
 * (MONAI ViT Linear layers built at unetr.py:78-89) for the bf16 precision mode, where LayerNorm / attention / GELU
 * epilogues and the optimizer's weight shadow already hold the operands as bf16.
 *   C[M,N] = epilogue(A[M,K] * Bop):  A bf16 [M,K] (k contiguous, pitch lda);
 *   b_kn = 0: B bf16 [N,K] (pitch ldb; forward y = x W^T);  b_kn = 1: B bf16 [K,N] (pitch ldb; dgrad dx = dy W).
 * K must be a multiple of 64; pitches multiples of 8 elements.  Outputs: fp32 C (pitch ldc; may be NULL) and/or
 * bf16 Cb (pitch ldcb; may be NULL); `pre`/`accumulate` need C.  Epilogue fields as in unetr_gemm_desc. */
typedef struct {
    int M, N, K, b_kn;
    long lda, ldb, ldc, ldcb;
    const float* bias;
    const float* res;
    long ldr;
    int res_mod;
    float* pre;
    const float* aux;
    long ldaux;
    int act;
    int accumulate;
    float alpha;
    /* tc_cout > 0: the output is a 2x2x2 stride-2 ConvTranspose3d result scattered in place (UnetrPrUpBlock / UnetrUpBlock,
     * unetr.py:99-174): row m is voxel (b, z, y, x) of the INPUT grid [*, tc_d, tc_h, tc_w], column n = tap * tc_cout + co (the
     * tap-major weight pack, kind 4 of unetr_conv3_pack_grouped), and the value goes to Cb[outvox(m, tap) * ldcb + co] with
     * outvox = (b, 2z + tap/4, 2y + (tap/2)%2, 2x + tap%2) of the output grid.  bf16 output only (C and pre NULL). */
    int tc_d, tc_h, tc_w, tc_cout;
    /* x3 != 0: bf16x3 precision mode through these entry points (what the LayerNorm-riding forms unetr_gemm_bf16_ln_fwd / _ln_bwd need):
     * A is fp32 [M,K], B fp32 (x3 = 1) or pre-split words (x3 = 2: unetr_split_words), both in the b_kn layout rule above; C fp32 only;
     * K % 32 == 0, pitches % 4 == 0.  UNETR_ERR_UNSUPPORTED when the LDS-DMA kernel declines the shape (use unetr_gemm + the plain
     * LayerNorm entry points then). */
    int x3;
} unetr_gemm_bf16_desc;
int unetr_gemm_bf16(const unetr_gemm_bf16_desc* d, const void* A, const void* B, float* C, void* Cb,
                    float* ws, size_t ws_bytes, void* stream);
/* fp32 -> bf16 round-to-nearest-even copy (weight shadows; torch .to(torch.bfloat16) semantics) */
int unetr_cast_bf16(const float* src, void* dst, long n, void* stream);
/* bf16x3 mode, weight gradients: fp32 [rows, cols] -> bf16 [3 rows, cols] stack of its (hi, lo) halves -- second == 0: [hi; hi; lo]
 * (the dY side), second == 1: [hi; lo; hi] (the X side) -- so that dY^T X over the stacked rows = hi*hi + hi*lo + lo*hi on the
 * bf16 grouped weight-gradient kernel (unetr_gemm_bf16_grouped_wgrad[_adamw]).  rows * cols % 8 == 0, 16-byte aligned. */
int unetr_split_stack_bf16(const float* src, void* dst, long rows, long cols, int second, void* stream);
/* every stack of a backward pass in one launch */
typedef struct { const float* src; void* dst; long rows, cols; int second; } unetr_split_problem;
int unetr_split_stack_bf16_grouped(const unetr_split_problem* probs, int n, void* stream);
/* out = a + b (fp32, n % 4 == 0, 16-byte aligned) and out_bf16 = bf16(out) (may be NULL): the sum autograd forms for a hidden
 * state with two consumers (unetr.py:197-201: hidden states 3, 6, 9 feed the next block AND encoder2-4) */
int unetr_add_cast_bf16(const float* a, const float* b, float* out, void* out_bf16, long n, void* stream);

/* Grouped launches for the work that is OFF the critical path of backward at batch 2: the weight gradients
 * dW_i[N_i,K_i] = dY_i[M_i,N_i]^T * X_i[M_i,K_i] of all transformer blocks (torch.nn.Linear backward, MONAI
 * ViT built at unetr.py:78-89) and the bias / position-embedding gradient column sums.  One launch covers up to
 * 48 problems (descriptors travel in the kernel-argument block), filling the chip without split-K slabs. */
typedef struct { const float* dy; const float* x; float* dw; int M, N, K; } unetr_grouped_problem;
int unetr_gemm_grouped_wgrad(const unetr_grouped_problem* probs, int n, int prec, void* stream);
/* the same grouped weight gradients on bf16-STORED dy / x (the pointers in unetr_grouped_problem then address bf16 data,
 * dense row-major [M,N] / [M,K]; M, N, K multiples of 8): LDS-DMA staging, transposing LDS reads for both operands */
int unetr_gemm_bf16_grouped_wgrad(const unetr_grouped_problem* probs, int n, void* stream);
/* x_bf16 != 0: x addresses bf16 data (the bf16 twin of a data gradient: fc1's bias gradient is summed from the same bf16 values its
 * weight gradient is formed from, and the fp32 copy of that gradient is never written) */
typedef struct { const void* x; float* out; long ld; int M, N, x_bf16; } unetr_colsum_problem;
int unetr_colsum_grouped(const unetr_colsum_problem* probs, int n, void* stream);

/* ---- 2x2x2 stride-2 transposed conv (nn.ConvTranspose3d, bias=False; unetr.py:99-174) ---------------
 * x: [B,D,H,W,Cin] pitch ldx; w: torch layout [Cin,Cout,2,2,2]; y: [B,2D,2H,2W,Cout] pitch ldy. */
int unetr_tconv_fwd(const float* x, long ldx, const float* w, float* y, long ldy,
                    int B, int D, int H, int W, int Cin, int Cout, int prec,
                    float* ws, size_t ws_bytes, void* stream);
int unetr_tconv_dgrad(const float* dy, long ldy, const float* w, float* dx, long ldx, int accumulate,
                      int B, int D, int H, int W, int Cin, int Cout, int prec,
                      float* ws, size_t ws_bytes, void* stream);
int unetr_tconv_wgrad(const float* x, long ldx, const float* dy, long ldy, float* dw,
                      int B, int D, int H, int W, int Cin, int Cout, int prec,
                      float* ws, size_t ws_bytes, void* stream);
/* Dedicated kernels for the same transposed conv at large-volume / small-channel layers (persistent workgroups over
 * 64-voxel tiles, LDS table of output-voxel bases, dy gathered voxel-major and read through transposing LDS loads).
 * Same arguments and results as unetr_tconv_fwd / unetr_tconv_wgrad; return "unsupported" (3) for shapes outside their
 * range (M = B*D*H*W < 2048, channel counts, alignment) -- the caller then uses the generic entry points above. */
int unetr_tconv2_fwd(const void* x, long ldx, const float* w, void* y, long ldy,
                     int B, int D, int H, int W, int Cin, int Cout, int prec,
                     float* ws, size_t ws_bytes, void* stream);
int unetr_tconv2_wgrad(const void* x, long ldx, const void* dy, long ldy, float* dw,
                       int B, int D, int H, int W, int Cin, int Cout, int prec,
                       float* ws, size_t ws_bytes, void* stream);
int unetr_tconv2_dgrad(const void* dy, long ldy, const float* w, void* dx, long ldx, int accumulate,
                       int B, int D, int H, int W, int Cin, int Cout, int prec,
                       float* ws, size_t ws_bytes, void* stream);
/* unetr_tconv2_wgrad without its reduce launch (see unetr_conv3_wgrad_parts): part [rows][Cin Cout 8] */
long unetr_tconv2_wgrad_rows(int B, int D, int H, int W, int Cin, int Cout);
int unetr_tconv2_wgrad_parts(const void* x, long ldx, const void* dy, long ldy, float* part, size_t part_bytes, long* rows_out,
                             int B, int D, int H, int W, int Cin, int Cout, int prec, void* stream);
int unetr_tconv2_fwd_supported(long M, int Cin, int Cout, long ldx, long ldy);
int unetr_tconv2_wgrad_supported(long M, int Cin, int Cout, long ldx, long lddy);


/* ---- the same attention core on bf16-STORED q/k/v (bf16 mode, head dim 64): qkv bf16 [B*L, 3*heads*64] as written by
 * unetr_gemm_bf16, out fp32 and/or bf16 [B*L, heads*64] (either may be NULL), lse [B, heads, L].  Backward: out_bf16 /
 * dout_bf16 bf16 [B*L, heads*64], writes dqkv_bf16 (required) and dqkv fp32 (optional), delta [B, heads, L] scratch.
 * Returns "unsupported" (3) for other head dims -- the caller then uses unetr_attention_fwd / _bwd on fp32 q/k/v. */
int unetr_attention_bf16_fwd(const void* qkv, float* out, void* out_bf16, float* lse, int B, int L, int heads, int dh,
                             float scale, void* stream);
int unetr_attention_bf16_bwd(const void* qkv, const void* out_bf16, const void* dout_bf16, const float* lse, float* dqkv,
                             void* dqkv_bf16, float* delta, int B, int L, int heads, int dh, float scale, void* stream);

/* ---- prefetch rider: weight bytes for the NEXT launch(es), read by spare workgroups of a small launch ---------------------------
 * The ViT Linear GEMMs at a few hundred token rows are one round of workgroups whose first K stages wait on HBM: their weights are
 * used once per pass and never survive in the Infinity Cache until the next use.  The launch just before such a GEMM (a LayerNorm,
 * the attention core) leaves most of the chip idle; the *_pf entry points below run the same kernels with extra workgroups, placed
 * after the work blocks, that only read up to two byte ranges [ptr[i], ptr[i] + bytes[i]) with plain 16-byte loads, so those lines
 * are cache hits for the following GEMM(s).  A rider writes nothing and takes no part in the work blocks' barriers or
 * reductions: results are bit-identical and workspaces are sized as without it.  Only whole 16-byte units inside a range are
 * read (ragged ends are skipped); ptr == NULL or bytes < 16 drops that range; pf == NULL or two empty ranges launch exactly the
 * grid of the plain entry point.  Ranges must be readable device memory for the duration of the launch.
 * (These entry points are additions: no existing signature moved, so UNETR_ABI_VERSION stays where it was -- a library built
 * before them lacks the symbols and is refused at load for that.) */
typedef struct { const void* ptr[2]; size_t bytes[2]; } unetr_prefetch;
int unetr_attention_bf16_fwd_pf(const void* qkv, float* out, void* out_bf16, float* lse, int B, int L, int heads, int dh,
                                float scale, void* stream, const unetr_prefetch* pf);
int unetr_attention_bf16_bwd_pf(const void* qkv, const void* out_bf16, const void* dout_bf16, const float* lse, float* dqkv,
                                void* dqkv_bf16, float* delta, int B, int L, int heads, int dh, float scale, void* stream,
                                const unetr_prefetch* pf);

/* The small transposed convs (Cin a multiple of 64, bf16 mode) run as plain unetr_gemm_bf16 calls on torch's own weight
 * matrix [Cin, Cout*8]; these two move between the GEMM-side matrix t / g [M, Cout*8] (column = co*8 + tap) and the
 * voxel-major tensor y / dy [B, 2D, 2H, 2W, Cout] (pitch ldy): the pixel shuffle that is left of the "transposed conv". */
int unetr_pixel_shuffle2(const float* t, void* y, long ldy, int B, int D, int H, int W, int Cout, int act16, void* stream);
int unetr_pixel_unshuffle2_bf16(const void* dy, long lddy, void* g_bf16, int B, int D, int H, int W, int Cout, int act16, void* stream);

/* ---- column sums: out[n] (+)= sum_m x[m*ld+n]  (bias / position-embedding gradients) ---------------- */
int unetr_colsum(const float* x, long ld, int M, int N, float* out, int accumulate,
                 float* ws, size_t ws_bytes, void* stream);

/* ---- LayerNorm (nn.LayerNorm(H), eps 1e-5, affine; MONAI TransformerBlock.norm1/2, ViT.norm) -------- */
int unetr_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y,
                        void* y_bf16 /* optional bf16 copy of y for unetr_gemm_bf16, or NULL; y itself may be NULL when only the bf16 copy is wanted */,
                        float* mean, float* rstd, int M, int H, float eps, void* stream);
/* dgamma == dbeta == NULL: only dx is produced and ws keeps the per-row-block partial sums, laid out
 * [ceil(M/4)][2][H] (dgamma row, dbeta row), for a later unetr_colsum_grouped over all LayerNorms of the step. */
int unetr_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean,
                        const float* rstd, float* dx, void* dx_bf16 /* optional bf16 copy of dx, or NULL */,
                        const float* dres /* optional, added to dx */, float* dgamma, float* dbeta,
                        int M, int H, float* ws, size_t ws_bytes, void* stream);
/* the same two launches carrying a prefetch rider (unetr_prefetch above; pf may be NULL) */
int unetr_layernorm_fwd_pf(const float* x, const float* gamma, const float* beta, float* y, void* y_bf16,
                           float* mean, float* rstd, int M, int H, float eps, void* stream, const unetr_prefetch* pf);
int unetr_layernorm_bwd_pf(const float* dy, const float* x, const float* gamma, const float* mean,
                           const float* rstd, float* dx, void* dx_bf16, const float* dres, float* dgamma, float* dbeta,
                           int M, int H, float* ws, size_t ws_bytes, void* stream, const unetr_prefetch* pf);

/* nn.LayerNorm backward (norm1 / norm2 of MONAI TransformerBlock) applied to dy = A . B, the data gradient of the Linear layer
 * that consumed the LayerNorm output (SABlock.qkv / MLPBlock.linear1): when that GEMM is cut into K slabs the LayerNorm kernel
 * sums the slabs itself (same order as the separate reduce launch: bit-identical), saving one launch per LayerNorm.  `d` must
 * describe a plain product (alpha 1, no bias / activation / residual / accumulate, ldc == N); C [M, N] is scratch; the remaining
 * arguments are those of unetr_layernorm_bwd (ln_ws = its ws). */
int unetr_gemm_bf16_ln_bwd(const unetr_gemm_bf16_desc* d, const void* A, const void* B, float* C,
                           const float* x, const float* gamma, const float* mean, const float* rstd,
                           float* dx, void* dx_bf16, const float* dres, float* dgamma, float* dbeta,
                           float* ln_ws, size_t ln_ws_bytes, float* ws, size_t ws_bytes, void* stream);

/* The forward counterpart: C = A . B + bias + res (MLPBlock.linear2 + the block's residual add) and nn.LayerNorm of C (norm1 of
 * the NEXT TransformerBlock) -- when the GEMM is cut into K slabs the LayerNorm kernel sums them, applies bias and residual,
 * writes C and normalises the row (bit-identical to the three separate launches).  `d`: bias / res allowed, no activation / pre /
 * accumulate, alpha 1, ldc == N.  y (fp32) and / or y_bf16 receive the normalised rows. */
int unetr_gemm_bf16_ln_fwd(const unetr_gemm_bf16_desc* d, const void* A, const void* B, float* C,
                           const float* gamma, const float* beta, float eps, float* y, void* y_bf16, float* mean, float* rstd,
                           float* ws, size_t ws_bytes, void* stream);
/* both LayerNorm-riding forms with a prefetch rider on their LayerNorm launch (pf may be NULL) */
int unetr_gemm_bf16_ln_bwd_pf(const unetr_gemm_bf16_desc* d, const void* A, const void* B, float* C,
                              const float* x, const float* gamma, const float* mean, const float* rstd,
                              float* dx, void* dx_bf16, const float* dres, float* dgamma, float* dbeta,
                              float* ln_ws, size_t ln_ws_bytes, float* ws, size_t ws_bytes, void* stream, const unetr_prefetch* pf);
int unetr_gemm_bf16_ln_fwd_pf(const unetr_gemm_bf16_desc* d, const void* A, const void* B, float* C,
                              const float* gamma, const float* beta, float eps, float* y, void* y_bf16, float* mean, float* rstd,
                              float* ws, size_t ws_bytes, void* stream, const unetr_prefetch* pf);

/* ---- multi-head self-attention core (MONAI SABlock.forward between qkv and out_proj) ----------------
 * qkv: [B*L, 3*Hd] with feature = which*Hd + head*dh + j;  out: [B*L, Hd] ("b h l d -> b l (h d)");
 * lse: [B, heads, L] log-sum-exp of the scaled scores (saved for backward). */
int unetr_attention_fwd(const float* qkv, float* out, void* out_bf16 /* optional bf16 copy, or NULL */, float* lse,
                        int B, int L, int heads, int dh, float scale, int prec, void* stream);
int unetr_attention_bwd(const float* qkv, const float* out, const float* dout, const float* lse,
                        float* dqkv, void* dqkv_bf16 /* optional bf16 copy, or NULL */, float* delta,
                        int B, int L, int heads, int dh, float scale, int prec, void* stream);

/* ---- 3x3x3 (pad 1) and 1x1x1 conv, stride 1, no bias (nn.Conv3d in MONAI UnetResBlock.conv1/2/3) ------
 * General-shape path: implicit GEMM through the MFMA GEMM family (im2col operand loaders, no im2col
 * buffer).  wpack comes from unetr_conv_pack_weight: mode 0 = forward [Cout][KV][Cin]; mode 1 = data
 * gradient (taps flipped, in/out swapped) [Cin][KV][Cout], to be used with Cin/Cout swapped. */
int unetr_conv_pack_weight(const float* w, float* wpack, int Cin, int Cout, int KS, int mode, void* stream);
int unetr_conv_gemm_fwd(const float* x, long ldx, const float* wpack, float* y, long ldy, int accumulate,
                        int B, int D, int H, int W, int Cin, int Cout, int KS, int prec,
                        float* ws, size_t ws_bytes, void* stream);
int unetr_conv_gemm_wgrad(const float* x, long ldx, const float* dy, long ldy, float* dw,
                          int B, int D, int H, int W, int Cin, int Cout, int KS, int prec,
                          float* ws, size_t ws_bytes, void* stream);

/* Dedicated 3x3x3 path (csrc/conv3.hip): LDS-staged halo windows, one HBM/L2 read per tile for all 27 taps.
 * wpack (element type follows prec) comes from unetr_conv3_pack_weight, sized by unetr_conv3_packed_bytes;
 * mode 0 = forward, mode 1 = data gradient (then call unetr_conv3_fwd with Cin/Cout swapped).  Cout % 16 == 0. */
size_t unetr_conv3_packed_bytes(int Cin, int Cout, int mode, int prec);
int unetr_conv3_pack_weight(const float* w, void* wpack, int Cin, int Cout, int mode, int prec, void* stream);
int unetr_conv3_fwd(const void* x, long ldx, const void* wpack, void* y, long ldy, int accumulate,
                    int B, int D, int H, int W, int Cin, int Cout, int prec, void* stream);
/* dy3/dw3 (both or neither): also produce the weight gradient dw3[Cout,Cin] of the 1x1x1 conv that shares the
 * input x (MONAI UnetResBlock.conv3 next to conv1) from its own output gradient dy3, inside the same pass. */
/* Fused forward of the first half of MONAI's UnetResBlock (unetr.py:90-98, :135-174): y = conv3x3x3(x) together with
 * its InstanceNorm statistics stats[B,Cout,2] = (mean, rstd), and -- when w3pack != NULL -- y3 = conv1x1x1(x) (the
 * block's conv3, which reads the same input) with stats3.  wpack from unetr_conv3_pack_weight(mode 0), w3pack from
 * unetr_conv3_pack_1x1.  Returns "unsupported" for shapes that do not run on the persistent kernel (caller then uses
 * unetr_conv3_fwd + unetr_gemm + unetr_instnorm_stats). */
int unetr_conv3_fwd_fused(const void* x, long ldx, const void* wpack, void* y, long ldy, float* stats,
                          const void* w3pack, void* y3, long ldy3, float* stats3, float eps,
                          int B, int D, int H, int W, int Cin, int Cout, int prec,
                          int x_f32 /* bf16 mode: x is the fp32 image (<= 16 channels), not a bf16 feature map */,
                          float* ws, size_t ws_bytes, void* stream);
/* The same launch without the statistics finalize: the InstanceNorm partial sums stay as rows part / part3 [B][rows][2][Cout]
 * (caller-allocated for UNETR_CONV3_MAX_ROWS rows; *rows_out = the rows this launch wrote, one per workgroup) and are reduced by
 * their consumer in its own prologue (unetr_instnorm_apply_fin) -- no finalize launch. */
#define UNETR_CONV3_MAX_ROWS 1024
int unetr_conv3_fwd_parts(const void* x, long ldx, const void* wpack, void* y, long ldy, float* part,
                          const void* w3pack, void* y3, long ldy3, float* part3, int* rows_out,
                          int B, int D, int H, int W, int Cin, int Cout, int prec, int x_f32, void* stream);
/* Data gradient dx[.,Cin] = conv3x3x3^T(dy[.,Cout]; w) of a conv whose input was lrelu(InstanceNorm(xn)) (UnetResBlock.conv2,
 * unetr.py:90-98 / :135-174 via MONAI), with the backward statistics of that norm formed in the epilogue: part [B][rows][2][Cin]
 * = per-workgroup sums of g and g*n, g = dx * lrelu'(n), n = (xn - mean) * rstd from stats [B][Cin][2].  Replaces the separate
 * reduction pass of unetr_instnorm_bwd over (dx, xn); consumed by unetr_instnorm_bwd_apply_fin(nsp = 2). */
int unetr_conv3_dgrad_stats(const void* dy, long lddy, const void* wpack_dgrad, void* dx, long lddx,
                            const void* xn, long ldxn, const float* stats, float* part, int* rows_out,
                            int B, int D, int H, int W, int Cin, int Cout, int prec, void* stream);
size_t unetr_conv3_packed_1x1_bytes(int Cin, int Cout, int prec);
int unetr_conv3_pack_1x1(const float* w3 /* [Cout,Cin] */, void* w3pack, int Cin, int Cout, int prec, void* stream);
/* Data gradient of the residual block's input in one launch: dx = conv3x3x3^T(dc1; w1) + conv1x1x1^T(dc3; w3)
 * (autograd of UnetResBlock.conv1 + conv3, both fed by the block input).  wpack_dgrad from unetr_conv3_pack_weight(mode 1)
 * of conv1's weight; w3 = conv3's weight [Cout, Cin] as stored; dc1 / dc3 [B,D,H,W,Cout] channels-last with pitches. */
int unetr_conv3_dgrad_fused(const void* dc1, long ld1, const void* wpack_dgrad, const void* dc3, long ld3, const float* w3,
                            const void* w3pack_t /* optional: kind-3 pack of w3 (unetr_conv3_pack_grouped); NULL = packed here from w3 */,
                            void* dx, long lddx, int B, int D, int H, int W, int Cin, int Cout, int prec,
                            float* ws, size_t ws_bytes, void* stream);
/* Query, no launch and no device: how a forward / data-gradient launch with >= 32 (bf16) / any (fp32, bf16x3) contraction channels
 * Cin and Cout produced channels is dispatched.  fuse: 0 plain, 1 statistics, 2 / 3 statistics + 1x1x1 branch (Cin > / <= one
 * k-block), 4 unetr_conv3_dgrad_fused, 5 unetr_conv3_dgrad_stats (the data gradients pass the conv's Cout as Cin here).
 * out[6] = {output tiles of 16 channels per workgroup, weight images in LDS, grid.x (= partial rows), grid.y, workgroups of that
 * kernel variant the chip holds at once, LDS bytes of its window and weight images}; grid.x * grid.y <= out[4] whenever the volume has fewer than 512 tiles.
 * (Addition: no existing signature moved, UNETR_ABI_VERSION stays.) */
int unetr_conv3_slab_dispatch(int B, int D, int H, int W, int Cin, int Cout, int prec, int fuse, int* out);
/* All weight re-packs of a step in one launch (descriptors in the kernel arguments, <= 64 per launch).  kind 0 / 1: what
 * unetr_conv3_pack_weight(mode 0 / 1) writes; kind 2: unetr_conv3_pack_1x1; kind 3: the transposed 1x1x1 layout that
 * unetr_conv3_dgrad_fused builds internally.  `out` buffers sized by unetr_conv3_packed_bytes / _packed_1x1_bytes. */
typedef struct { const float* w; void* out; int Cin, Cout, kind; } unetr_pack_problem;
int unetr_conv3_pack_grouped(const unetr_pack_problem* probs, int n, int prec, void* stream);
/* (mean, rstd) from InstanceNorm partial sums part[B][nchunk][2][C] (sum, sum of squares) */
int unetr_instnorm_stats_finalize(const float* part, int nchunk, int B, long V, int C, float eps, float* stats, void* stream);
int unetr_conv3_wgrad(const void* x, long ldx, const void* dy, long ldy, float* dw,
                      const void* dy3, long ldy3, float* dw3,
                      int B, int D, int H, int W, int Cin, int Cout, int prec, int x_f32 /* as in unetr_conv3_fwd_fused */,
                      float* ws, size_t ws_bytes, void* stream);
/* The same weight gradients WITHOUT their reduce launch: the per-workgroup partial sums stay in `part` -- [rows][27 Cin Cout] followed,
 * when dy3 is given, by [rows][Cin Cout]; *rows_out = rows written (= unetr_conv3_wgrad_rows for an unlimited buffer; fewer when
 * part_bytes forces it) -- and are summed later by unetr_reduce_rows_grouped together with every other weight-gradient reduction
 * of the backward pass. */
long unetr_conv3_wgrad_rows(int B, int D, int H, int W, int Cin, int Cout, int prec, int x_f32, int has3);
int unetr_conv3_wgrad_parts(const void* x, long ldx, const void* dy, long ldy, const void* dy3, long ldy3,
                            float* part, size_t part_bytes, long* rows_out, int B, int D, int H, int W, int Cin, int Cout, int prec,
                            int x_f32, void* stream);
/* dst[i] = sum over rows g of part[g][i], i < n, for every problem, in one launch (fixed summation order) */
typedef struct { const float* part; float* dst; long n; int rows; } unetr_reduce_problem;
int unetr_reduce_rows_grouped(const unetr_reduce_problem* probs, int n, void* stream);
/* probe of the ds_read_b64_tr_b16 lane map used by the bf16 weight-gradient kernel (test hook) */
int unetr_debug_tr16(const void* in_u16_64x64, void* out_u16_64x4, void* stream);

/* ---- InstanceNorm3d(affine=False, eps 1e-5) + LeakyReLU(0.01) + residual add -------------------------
 * stats: [B, C, 2] = (mean, rstd). */
int unetr_instnorm_stats(const void* x, long ld, int B, long V, int C, float eps, float* stats,
                         float* ws, size_t ws_bytes, int act16, void* stream);
/* y = lrelu?(norm(x;sa) [+ norm(x2;sb)]) */
int unetr_instnorm_apply(const void* x, long ldx, const float* sa, const void* x2, long ldx2, const float* sb,
                         void* y, long ldy, int B, long V, int C, int lrelu, int act16, void* stream);
/* unetr_instnorm_apply with the statistics finalize folded into the kernel's prologue: part_a / part_b = the partial rows
 * [B][rows][2][C] of the conv launches that produced x / x2; stats_a / stats_b [B][C][2] are WRITTEN (for the backward kernels).
 * "unsupported" for C > 128 or unaligned rows: the caller then runs unetr_instnorm_stats_finalize + unetr_instnorm_apply. */
int unetr_instnorm_apply_fin(const void* x, long ldx, const float* part_a, int rows_a, const void* x2, long ldx2,
                             const float* part_b, int rows_b, float* stats_a, float* stats_b, float eps,
                             void* y, long ldy, int B, long V, int C, int lrelu, int act16, void* stream);
/* the apply half of unetr_instnorm_bwd reading partial sums part [B][nrows][nsp][C] (nsp 2: rows of unetr_conv3_dgrad_stats,
 * single form only; nsp 3: the reduction pass's rows) and finalizing them in its prologue */
int unetr_instnorm_bwd_apply_fin(const void* dy, long lddy, const void* x, long ldx, const float* sa,
                                 const void* x2, long ldx2, const float* sb, const float* part, int nrows, int nsp,
                                 void* dx, long lddx, void* dx2, long lddx2, int B, long V, int C, int lrelu, int act16, void* stream);
/* The block end of the residual block that reads the IMAGE (encoder1, unetr.py:90-98; <= 4 input channels): its 1x1x1 branch
 * c3 = conv1x1x1(img; w3 [C][Cin]) is formed per voxel from the fp32 image [B][V][Cin] instead of being stored and re-read, forward
 * (y = lrelu(norm(x) + norm(c3)); part_b = the partial rows of c3's statistics from unetr_conv3_fwd_parts, which then takes
 * y3 = NULL) and backward (dx of the 3x3x3 branch; the branch's weight gradient as partial rows dw3_part [*rows_out][C][Cin],
 * caller-allocated for UNETR_IN_IMG_MAX_ROWS rows, summed by unetr_reduce_rows_grouped; ws >= B * 1024 * 3 * C floats). */
#define UNETR_IN_IMG_MAX_ROWS 512
int unetr_instnorm_apply_fin_img(const void* x, long ldx, const float* part_a, int rows_a, const float* img, int Cin, const float* w3,
                                 const float* part_b, int rows_b, float* stats_a, float* stats_b, float eps,
                                 void* y, long ldy, int B, long V, int C, int lrelu, int act16, void* stream);
int unetr_instnorm_bwd_img(const void* dy, long lddy, const void* x, long ldx, const float* sa, const float* img, int Cin,
                           const float* w3, const float* sb, void* dx, long lddx, float* dw3_part, int* rows_out,
                           int B, long V, int C, int lrelu, float* ws, size_t ws_bytes, int act16, void* stream);
/* backward of y = lrelu?(norm(x) [+ norm(x2)]): writes dx (and dx2). */
int unetr_instnorm_bwd(const void* dy, long lddy, const void* x, long ldx, const float* sa,
                       const void* x2, long ldx2, const float* sb, void* dx, long lddx, void* dx2, long lddx2,
                       int B, long V, int C, int lrelu, float* ws, size_t ws_bytes, int act16, void* stream);

/* ---- layout moves --------------------------------------------------------------------------------- */
/* NCDHW [B,C,V] <-> channels-last [B,V,C] (pitch ld) */
int unetr_nchw_to_nhwc(const float* x /* fp32 NCDHW */, void* y /* feature map */, long ldy, int B, int C, long V, int act16, void* stream);
int unetr_nhwc_to_nchw(const void* x /* feature map */, long ldx, float* y /* fp32 NCDHW */, int B, int C, long V, int accumulate, int act16, void* stream);
/* einops "b c (h p1) (w p2) (d p3) -> b (h w d) (p1 p2 p3 c)" (MONAI PatchEmbeddingBlock, perceptron) */
/* patches (fp32) and / or patches_bf16 (the bf16 GEMM operand) may be NULL, not both */
int unetr_patch_gather(const float* x, float* patches, void* patches_bf16, int B, int C, int D, int H, int W, int P, void* stream);
/* y[i] += inc[i], i < n: AdamW's per-parameter step counters (device-resident so that the step can be a hipGraph) */
int unetr_counter_add(float* y, const float* inc, int n, void* stream);
/* ---- AdamW hyper-parameter row: four floats in DEVICE memory, {lr, weight_decay, t, reserved}, one row per param group.  The
 * optimizer kernels that are given a row read lr / weight_decay from it when they run, not when they are launched: a captured step
 * follows a learning-rate change without being captured again.  t = number of optimizer steps taken (a float like the per-parameter
 * counters: exact to 2^24 steps).
 * unetr_lr_schedule (passed BY VALUE into the launch): lr = max(min_lr, base_lr * f(s)), s = t before the increment -- the first
 * step uses f(0), as torch.optim.lr_scheduler does.  kind 0 constant: f = 1.  kind 1 warm-up + cosine: s < warmup: f = s / max(1, warmup),
 * else f = 0.5 (1 + cos(pi min(1, (s - warmup) / max(1, total - warmup)))).  kind 2 poly (nnU-Net): f = (1 - min(s, total) / total)^power,
 * total > 0.  f is computed in double and lr rounded once to float. */
typedef struct { int kind; float base_lr, min_lr, warmup, total, power; } unetr_lr_schedule;
/* unetr_counter_add that also keeps a hyper row, in the SAME launch (the captured step gains no launch): one thread sets
 * row.lr from the schedule at row.t (s == NULL: lr is left as the host wrote it), then row.t += 1. */
int unetr_counter_add_lr(float* y, const float* inc, int n, float* hyper_row, const unetr_lr_schedule* s, void* stream);
/* stream-ordered write of the row fields selected by `fields` (bit 0: lr, bit 1: weight_decay, bit 2: t) from by-value arguments:
 * one single-thread launch, no host synchronisation, no staging buffer */
int unetr_adamw_hyper_set(float* hyper_row, int fields, float lr, float weight_decay, float t, void* stream);
/* y[r, 0:cols] (+)= a[r, 0:cols] for row-pitched matrices (skip -> concat buffer, gradient sums) */
int unetr_copy_rows(void* y, long ldy, const void* a, long lda, long rows, int cols, int accumulate, int act16, void* stream);

/* ---- 1x1x1 out conv with bias, NCDHW logits (MONAI UnetOutBlock; unetr.py:175,207) ------------------ */
int unetr_outconv_fwd(const void* x, long ldx, const float* w, const float* bias, float* logits,
                      int B, long V, int Cin, int Cout, int act16, void* stream);
int unetr_outconv_bwd(const float* dlogits, const void* x, long ldx, const float* w, void* dx, long lddx,
                      float* dw, float* dbias, int B, long V, int Cin, int Cout,
                      float* ws, size_t ws_bytes, int act16, void* stream);

/* decoder2's block end folded into the out conv (reference: UnetrUpBlock's UnetResBlock followed by UnetOutBlock,
 * /root/reference/unetr.py:165-175,206-207): out = lrelu(IN(c2) + IN(c3)) is formed per voxel and never stored.
 * unetr_outconv_in_fwd: logits [B][Cout][V] from c2 / c3 [B][V][C] and their InstanceNorm partial rows; writes stats_a / stats_b.
 * unetr_outconv_in_bwd: dout = W^T dlogits (stored, pitch lddo), the InstanceNorm backward partial rows in_part [B][rows][3][C]
 * (rows = unetr_outconv_in_bwd_rows; feed unetr_instnorm_bwd_apply_fin with nsp = 3), dw [Cout][C], dbias [Cout].
 * UNETR_ERR_UNSUPPORTED (Cout > 4, C > 16, ...) = run the unfused sequence. */
int unetr_outconv_in_fwd(const void* c2, long ld2, const float* part_a, int rows_a, const void* c3, long ld3, const float* part_b,
                         int rows_b, float* stats_a, float* stats_b, float eps, const float* w, const float* bias, float* logits,
                         int B, long V, int C, int Cout, int act16, void* stream);
long unetr_outconv_in_bwd_rows(int B, long V, int C, int act16);
int unetr_outconv_in_bwd(const float* dlogits, const void* c2, long ld2, const float* sa, const void* c3, long ld3, const float* sb,
                         const float* w, void* dout, long lddo, float* in_part, float* dw, float* dbias,
                         int B, long V, int C, int Cout, float* ws, size_t ws_bytes, int act16, void* stream);

/* ---- DiceCELoss (unetr_segmentation_3d.py:404 and :477-482) -------------------------------------------
 * sigmoid_multilabel = 0: DiceCELoss(to_onehot_y=True, softmax=True); label [B,V] float-valued class ids.
 * sigmoid_multilabel = 1: DiceCELoss(to_onehot_y=False, sigmoid=True); label [B,C,V] float multi-label mask; the
 *   CE term is softmax cross entropy against argmax_c(label) (MONAI 0.6.0 DiceCELoss.ce with equal channel counts).
 * logits [B,C,V] NCDHW.  out[0]=loss, out[1]=dice term, out[2]=ce term.
 * coef: [B*C*2] per-(b,c) Dice gradient coefficients kept for backward. */
int unetr_dicece_fwd(const float* logits, const float* label, int B, int C, long V, int sigmoid_multilabel,
                     float smooth_nr, float smooth_dr, float* out, float* coef, float* ws, size_t ws_bytes, void* stream);
int unetr_dicece_bwd(const float* logits, const float* label, const float* coef, const float* dloss,
                     float* dlogits, int B, int C, long V, int sigmoid_multilabel, void* stream);

/* ---- segmentation loss family: loss = lambda_region * R + lambda_voxel * X (csrc/seg_loss.hip) -------------
 * logits [B,C,V] fp32, 1 <= C <= 16 (else UNETR_ERR_UNSUPPORTED).  multilabel = 0: label [B,V] float class ids, p = softmax over
 * the channels, y = one_hot(label); multilabel = 1: label [B,C,V] float mask, p = sigmoid.  Per (b,c): I = sum p*y, P = sum p,
 * G = sum y (p^2 / y^2 with squared_pred; dice and jaccard only).  The region term runs over all channels, or 1..C-1 with
 * include_background = 0 (C >= 2), as a mean over (b, channel); batch = 1 pools I, P, G over b first.
 *   DICE     f = 1 - (2I + nr) / (G + P + dr)
 *   JACCARD  f = 1 - (2I + nr) / (2(G + P - I) + dr)
 *   TVERSKY  f = 1 - (I + nr) / (I + alpha (P - I) + beta (G - I) + dr)
 *   GDL      per item f = 1 - (2 sum_c w_c I_c + nr) / (sum_c w_c (G_c + P_c) + dr), w_c = 1/G_c^2, 1/G_c or 1 (w_type); a channel
 *            with G_c = 0 takes the item's largest finite weight (0 when there is none); w is a constant of the gradient
 * The voxel term: CE = softmax cross entropy over all channels against the label (multilabel: against argmax_c(mask), first
 * maximum), with class_weight[C] (device pointer or NULL; one-hot mode only) by torch's rule sum w_y (-log p_y) / sum w_y.  FOCAL =
 * sigmoid focal loss of the raw logits z against the target t, exp(gamma * logsigmoid(-z (2t - 1))) * bce(z, t) * class_weight[c],
 * as the plain mean over (b, included channels, v).  has_ignore (one-hot mode only): a voxel whose label equals ignore_index adds
 * to no sum, the voxel means divide by the count of the others (at least one per call), and its gradient is zero.
 * unetr_segloss_fwd: out[0] = loss, out[1] = R, out[2] = X; coef [B*C*3 + 1] floats kept for backward: per (b,c) the numbers
 *   (a, b, k) of d(lambda_region R)/dp_c(v) = a y + b p + k, then the factor of the voxel term's gradient.  ws: 16-byte aligned,
 *   unetr_segloss_workspace_bytes (0 for a descriptor that is refused).  Fixed-order partial sums, finalized by one block in
 *   double: reproducible run to run, no float atomics.
 * unetr_segloss_bwd: dlogits = *dloss (device scalar; NULL = 1) * dloss/dlogits, every element written.
 * Launches only: no allocation, no host synchronisation.  (Additions: no existing signature moved, UNETR_ABI_VERSION stays.) */
enum { UNETR_SEGLOSS_REGION_NONE = 0, UNETR_SEGLOSS_REGION_DICE = 1, UNETR_SEGLOSS_REGION_JACCARD = 2, UNETR_SEGLOSS_REGION_TVERSKY = 3,
       UNETR_SEGLOSS_REGION_GDL = 4 };
enum { UNETR_SEGLOSS_VOXEL_NONE = 0, UNETR_SEGLOSS_VOXEL_CE = 1, UNETR_SEGLOSS_VOXEL_FOCAL = 2 };
enum { UNETR_SEGLOSS_W_SQUARE = 0, UNETR_SEGLOSS_W_SIMPLE = 1, UNETR_SEGLOSS_W_UNIFORM = 2 };
typedef struct unetr_segloss_desc {
    int B, C;
    long V;
    int multilabel, region, voxel;
    int include_background, squared_pred, batch, w_type;
    int has_ignore, ignore_index;
    float smooth_nr, smooth_dr, alpha, beta, gamma, lambda_region, lambda_voxel;
    const float* class_weight;
} unetr_segloss_desc;
size_t unetr_segloss_workspace_bytes(const unetr_segloss_desc* d);
int unetr_segloss_fwd(const unetr_segloss_desc* d, const float* logits, const float* label, float* out, float* coef,
                      void* ws, size_t ws_bytes, void* stream);
int unetr_segloss_bwd(const unetr_segloss_desc* d, const float* logits, const float* label, const float* coef,
                      const float* dloss, float* dlogits, void* stream);

/* ---- validation side (unetr_segmentation_3d.py:103-132) -------------------------------------------------
 * unetr_sw_accumulate / unetr_sw_finalize: the blending step of monai.inferers.sliding_window_inference (MONAI 0.6.0,
 * called at :110): out[c, z0+z, y0+y, x0+x] += w * seg[c,z,y,x], count[...] += w for ONE window of ONE volume
 * (out / count point at that volume: [C,D,H,W] and [D,H,W]; importance = NULL means w = 1, mode="constant"), then
 * out[b,c,v] /= count[b,v].  One launch per window, in MONAI's window order.
 * unetr_dice_counts: the sums behind monai.metrics.DiceMetric (:485-486): counts[b][c] = (sum pred*y, sum pred, sum y).
 * from_logits = 1: pred = one_hot(argmax_c logits[B,C,V]) and y = class ids [B,V] (AsDiscrete(argmax, to_onehot) at
 * :405-406 fused in); from_logits = 0: pred and y are [B,C,V] (already discrete) tensors. */
int unetr_sw_accumulate(const float* seg, const float* importance, float* out, float* count, int C,
                        int rz, int ry, int rx, int D, int H, int W, int z0, int y0, int x0, void* stream);
int unetr_sw_finalize(float* out, const float* count, int B, int C, long V, void* stream);
int unetr_dice_counts(const float* pred, const float* y, int B, int C, long V, int from_logits, double* counts,
                      float* ws, size_t ws_bytes, void* stream);
/* Batched, table-driven form of the same blending (SlidingWindowInferer): one forward batch of up to UNETR_SW_MAX_BATCH windows
 * is one ROW of a device-resident window table, and the volume is described by a device-resident unetr_sw_volume, so no launch
 * carries a volume size or a window position in its arguments -- a hipGraph of advance -> gather -> forward -> accumulate serves
 * every volume.  A table row is UNETR_SW_ROW_INTS ints: [active, 0, 0, 0, then (b, z, y, x) per slot]; z, y, x are window
 * corners in the PADDED volume [D, H, W] (a volume smaller than the window is padded: input voxel = padded voxel - (pz, py, px)).
 * Every kernel reads row `cursor`; a cursor outside [0, rows), a slot whose window does not lie inside the padded volume of an
 * existing batch item, and a channel count that differs from the descriptor's make the launch (or that slot) a no-op.
 *   unetr_sw_advance          cursor += 1 (device-side, like AdamW's step counters: the row is chosen inside the graph)
 *   unetr_sw_gather_batch     dst [n, Cin, rz, ry, rx] = the windows of the row; voxels outside the stored input [B, Cin, Di, Hi, Wi]
 *                             -- and all of an inactive slot -- read cval (F.pad(mode="constant") fused in)
 *   unetr_sw_accumulate_batch out / count += the active windows of the row, seg [n, C, rz, ry, rx], in ONE launch.  Windows of a
 *                             row overlap: each output voxel is owned by the thread of the first active slot that covers it, which
 *                             adds the covering slots in slot order with the fp32 operations of unetr_sw_accumulate -- the result
 *                             is bit-identical to one unetr_sw_accumulate launch per window in slot order.  No atomics.
 *   unetr_sw_finalize_post    v = out / count (out [B, C, V], count [B, V]) and, in the same pass, post = 0: out = v;
 *                             1: out = one_hot(argmax_c v); 2: dst [B, V] = argmax_c v as float (out is left as sums);
 *                             3: out = (v >= 0), i.e. sigmoid(v) >= 0.5.  argmax takes the first maximal channel; post 1 / 2
 *                             need C <= 16.
 * Mirror test-time augmentation and ensembling (per window, the project's own semantics -- DESIGN.md section 18):
 *   row header int 1          the row's flip mask (bit 0 = z, bit 1 = y, bit 2 = x; 0 = none).  unetr_sw_gather_batch hands the
 *                             forward every window of the row mirrored along those axes (the mirror acts on the gathered, padded
 *                             window), and unetr_sw_accumulate_batch reads seg at the mirrored position, so the prediction is
 *                             blended un-flipped.  The importance map is indexed by the position in the VOLUME, never mirrored.
 *   activation                trailing descriptor field, read at run time by unetr_sw_accumulate_batch: 0 blends seg as it is,
 *                             1 softmax over the C channels of each window voxel, 2 sigmoid per element.
 *   unetr_sw_rewind           cursor = -1 (device-side): the next model of an ensemble walks the table again, out / count persist
 *   unetr_sw_finalize_post_thr  unetr_sw_finalize_post whose post = 3 stores (v >= threshold): 0 for blended logits, 0.5 for
 *                             blended sigmoid probabilities.  unetr_sw_finalize_post is threshold 0.
 * An all-zero header and activation are the behaviour described above, bit for bit.
 * (Additions: no existing signature moved, UNETR_ABI_VERSION stays.) */
#define UNETR_SW_MAX_BATCH 16
#define UNETR_SW_ROW_INTS (4 + 4 * UNETR_SW_MAX_BATCH)
typedef struct {
    const float* in; float* out; float* count; const int* table;
    int B, Cin, C;
    int Di, Hi, Wi;       /* stored input extents */
    int D, H, W;          /* padded extents (out, count, window corners) */
    int pz, py, px;       /* low-side padding */
    float cval;
    int rows, cursor;
    int activation;       /* 0 none, 1 softmax over channels, 2 sigmoid: applied to seg inside unetr_sw_accumulate_batch (a trailing
                             addition: a zero-initialised struct keeps the plain blend) */
} unetr_sw_volume;
int unetr_sw_advance(unetr_sw_volume* vol, void* stream);
int unetr_sw_gather_batch(const unetr_sw_volume* vol, float* dst, int n, int Cin, int rz, int ry, int rx, void* stream);
int unetr_sw_accumulate_batch(const unetr_sw_volume* vol, const float* seg, const float* importance, int n, int C,
                              int rz, int ry, int rx, void* stream);
int unetr_sw_finalize_post(float* out, const float* count, float* dst, int B, int C, long V, int post, void* stream);
int unetr_sw_rewind(unetr_sw_volume* vol, void* stream);
int unetr_sw_finalize_post_thr(float* out, const float* count, float* dst, int B, int C, long V, int post, float threshold,
                               void* stream);
/* unetr_hausdorff: monai.metrics.HausdorffDistanceMetric (MONAI 0.6.0, distance_metric="euclidean", :495-496) per item and
 * class: out[b][c - c0] (float64, [B][C-c0]) for the classes c0 <= c < C (c0 = 1: include_background=False).  pred / y as in
 * unetr_dice_counts (from_logits fuses argmax + one-hot; otherwise a voxel is in a mask where its value == 1).  use_percentile = 0
 * takes the max, 1 takes np.percentile(q * 100) (linear); directed = 1 returns d(pred -> gt) only.  Volumes [B,C,D,H,W] with
 * C <= 32, D, H, W <= 512.  ws holds unetr_hausdorff_workspace_bytes(B, C, D, H, W, group, use_percentile) bytes: 8 B per voxel
 * of the batch plus, per slot of the (b, c) group processed together, 9 B per voxel of one volume (8 B more per histogram bin
 * with percentiles, (D-1)^2+(H-1)^2+(W-1)^2+1 bins).  No host synchronisation. */
size_t unetr_hausdorff_workspace_bytes(int B, int C, int D, int H, int W, int group, int use_percentile);
int unetr_hausdorff(const float* pred, const float* y, int B, int C, int D, int H, int W, int c0, int from_logits,
                    int use_percentile, double q, int directed, double* out, void* ws, size_t ws_bytes, int group, void* stream);
/* unetr_surface_metrics: every surface metric of one (pred, gt) batch from ONE spacing-aware exact distance transform, in the
 * units of spacing[3] (float64 per step along D, H, W; host memory, each finite and > 0).  Same front end, edge rule and limits as
 * unetr_hausdorff.  input_form 0: one-hot float32 [B,C,D,H,W] for both (mask = value == 1); 1: float32 logits [B,C,D,H,W] and
 * float32 class ids [B,1,D,H,W]; 2: uint8 class ids [B,1,D,H,W] for both.  percentiles: npct <= 8 fractions in [0, 1] (host),
 * np.percentile's linear rule; thresholds: C - c0 tolerances, one per evaluated class (host), or NULL.
 * out (float64, device) is [8 + 2 * npct][B * (C - c0)]: edge counts n_pred, n_gt; max d(P->G), max d(G->P); mean d(P->G),
 * mean d(G->P); #(d(P->G) <= tau_c), #(d(G->P) <= tau_c); then the npct percentiles of d(P->G) and those of d(G->P).  A direction
 * without query edges gives nan for max / mean / percentile; one with query edges but nothing to measure to gives inf / inf /
 * nan.  Sums are reduced in a fixed order: two calls on the same input give the same bits.  ws holds
 * unetr_surface_metrics_workspace_bytes(B, C, D, H, W, group, npct) bytes: 8 B per voxel of the batch plus, per slot, 17 B per
 * voxel of one volume + 8752 B (+ 32 KiB with percentiles).  No host synchronisation.
 * (Additions: no existing signature moved, UNETR_ABI_VERSION stays.) */
size_t unetr_surface_metrics_workspace_bytes(int B, int C, int D, int H, int W, int group, int npct);
int unetr_surface_metrics(const void* pred, const void* y, int B, int C, int D, int H, int W, int c0, int input_form,
                          const double* spacing, const double* percentiles, int npct, const double* thresholds, double* out,
                          void* ws, size_t ws_bytes, int group, void* stream);

/* ---- ranking pre-training losses (unetr_ranking_pretraining_3d.py:59-133 triplet construction, :202-217 BTLoss,
 * :219-236 ContrastiveLoss), fused: feat is the NCDHW feature map [4, C, S1, S2, S3] (2 volumes x 2 transforms: enc4 in
 * the "feat" stage, logits in the "recon" stage), slice_dim in {2,3,4} as in the reference, init_idx the random slice
 * offset the reference draws with np.random.choice (injected for determinism).  kind 0 = Bradley-Terry, 1 = contrastive.
 * W [C,16,16] keeps dL/d<v_i,v_j> for backward; dfeat must be zero-filled by the caller (only the 16 slices are written). */
size_t unetr_ranking_workspace_floats(int C, int S1, int S2, int S3, int slice_dim);
int unetr_ranking_loss_fwd(const float* feat, int C, int S1, int S2, int S3, int slice_dim, int init_idx,
                           float temperature, int kind, float* loss, float* W, float* ws, size_t ws_floats, void* stream);
int unetr_ranking_loss_bwd(const float* feat, int C, int S1, int S2, int S3, int slice_dim, int init_idx,
                           const float* W, const float* dloss, float* dfeat, void* stream);

/* ---- GPU-resident training augmentation (csrc/augment.hip; unetr_segmentation_3d.py:322-476) ----
 * VolumeCache.add: unetr_aug_prep scales img [C,D,H,W] in place (scale_mode 1: ScaleIntensityRanged(clip=True) with the float32
 * constants a_min, a_range = a_max - a_min, b_range = b_max - b_min, b_min, b_max; 2: img - a_min; 0: none), folds the bounding
 * box of any_c(img > 0) into box[6] (z0, y0, x0, z1, y1, x1 inclusive; caller fills 0x7fffffff x3, -1 x3) when do_box, and sets
 * *flag where a value of lbl [L,D,H,W] is not an integer in 0..255.  unetr_aug_crop copies a box: image float32, label uint8.
 * unetr_aug_index_count / _scatter: the foreground (any_l(lbl != 0)) and background (!fg && any_c(img > thr)) voxel lists of
 * monai map_binary_to_indices, int32 in ascending ravel order; count writes the totals to ws[ws_ints - 2 .. ws_ints - 1].
 * RandCropAugment: vols is a DEVICE table of int64 rows (img ptr, lbl ptr, fg ptr, nfg, bg ptr, nbg, C, L, D, H, W, 0);
 * state (DEVICE int64: call counter, cursor, len(order), 0) is advanced by unetr_aug_sample, which writes params [B][8] (int32:
 * volume, corner z, y, x, flip mask, k, shift flag, offset as float bits) from Philox4x64-10 draws.  unetr_aug_gather maps every
 * voxel of x [B,C,S0,S1,S2] and y [B,L,S0,S1,S2] (float32) back to the volume; normalize adds NormalizeIntensity(nonzero=True,
 * channel_wise=True) per sample with ws of unetr_aug_gather_ws_bytes.  No host synchronisation.
 * Random rotation and zoom (this project's own semantics): unetr_aug_sample_affine draws what
 * unetr_aug_sample draws, from the same Philox words, and from blocks 3 and 4 of each sample the DEVICE table affine [B][16]
 * (float32: flag 0 / 1, angle about spatial axis 0, 1, 2, zoom of axis 0, 1, 2, M [3][3] row-major; M = R0 R1 R2 diag(1 / zoom)
 * in double from the stored float32 angles and zooms; an unflagged row holds zero angles, unit zooms and the identity).
 * unetr_aug_gather_affine is unetr_aug_gather for the unflagged rows, bit for bit; an output voxel of a flagged row, at crop
 * position p behind rot90 and the flips, reads the whole volume at c0 + (S - 1) / 2 + M (p - (S - 1) / 2): image trilinear,
 * label nearest (floor(src + 0.5)), taps outside the volume clamped to the border, float32 arithmetic in one fixed order with
 * no contraction (csrc/augment.hip: aug_affine_taps).  Volume extents up to 2^24.  Its workspace has its own query. */
typedef struct {
    int B, num_samples, C, L, S0, S1, S2;
    int sampling;                     /* 0 RandCropByPosNegLabeld, 1 RandSpatialCropSamplesd, 2 RandCropByLabelClassesd (below) */
    int ax0, ax1;                     /* rot90 spatial axes (S[ax0] == S[ax1]) */
    int max_k, normalize;
    double pos_ratio;                 /* pos / (pos + neg) */
    double flip_prob[3];
    double rot90_prob, shift_prob, shift_lo, shift_hi;
    unsigned long long seed;
} UnetrAugDesc;
long unetr_aug_index_ws_ints(long V);
int unetr_aug_prep(float* img, const float* lbl, int C, int L, int D, int H, int W, int scale_mode, float a_min, float a_range,
                   float b_range, float b_min, float b_max, int do_box, int* box, int* flag, void* stream);
int unetr_aug_crop(const float* img, const float* lbl, int C, int L, int D, int H, int W, int z0, int y0, int x0, int d, int h,
                   int w, float* oimg, unsigned char* olbl, void* stream);
int unetr_aug_index_count(const float* img, const unsigned char* lbl, int C, int L, long V, float thr, int* ws, size_t ws_ints,
                          void* stream);
int unetr_aug_index_scatter(const float* img, const unsigned char* lbl, int C, int L, long V, float thr, const int* ws,
                            size_t ws_ints, int* fg, int* bg, void* stream);
int unetr_aug_sample(const UnetrAugDesc* d, const long long* vols, int nvol, const int* order, long long* state, int* params,
                     void* stream);
size_t unetr_aug_gather_ws_bytes(const UnetrAugDesc* d);
int unetr_aug_gather(const UnetrAugDesc* d, const long long* vols, int nvol, const int* params, float* x, float* y, void* ws,
                     size_t ws_bytes, void* stream);
typedef struct {
    double prob;                      /* per sample */
    double rotate[3];                 /* the angle about spatial axis a is uniform in [-rotate[a], rotate[a]] (radians) */
    double zoom_lo, zoom_hi;          /* 0 < zoom_lo <= zoom_hi; a zoom z > 1 makes structures z times larger */
    int zoom_per_axis;                /* 0: one zoom for the three axes, 1: one draw per axis */
} UnetrAugAffineDesc;
int unetr_aug_sample_affine(const UnetrAugDesc* d, const UnetrAugAffineDesc* a, const long long* vols, int nvol, const int* order,
                            long long* state, int* params, float* affine, void* stream);
size_t unetr_aug_gather_affine_ws_bytes(const UnetrAugDesc* d);
int unetr_aug_gather_affine(const UnetrAugDesc* d, const long long* vols, int nvol, const int* params, const float* affine,
                            float* x, float* y, void* ws, size_t ws_bytes, void* stream);
/* Intensity augmentation on x after the gather (this project's own semantics, DESIGN.md section 12: nnU-Net's choice of
 * operations, MONAI's formulas, no bit parity with either): Gaussian blur, Gaussian noise, brightness, contrast, gamma, in that
 * order, each with its own probability per sample; y is not touched.  unetr_aug_intensity_sample, launched BEFORE
 * unetr_aug_sample (it reads state[0] and writes no state), draws from Philox blocks 5..7 of each sample the DEVICE table
 * [B][16] (int32, floats as their bits: flag bits noise 1 / blur 2 / brightness 4 / contrast 8 / gamma 16, noise std, blur sigma
 * of axis 0, 1, 2, brightness factor, contrast factor, gamma, low and high word of the call counter, six zeros; an unflagged
 * operation holds std 0, sigma 0, factor 1, gamma 1).  unetr_aug_intensity_apply runs the passes from such a table: launches
 * only, fixed grids, ws of unetr_aug_intensity_ws_bytes (16-byte aligned), no float atomics.  Statistics are per (sample,
 * channel) over the crop; sigma <= 2.  prob / lo / hi below are indexed noise std, blur sigma, brightness, contrast, gamma. */
typedef struct {
    double prob[5], lo[5], hi[5];
} UnetrAugIntensityDesc;
int unetr_aug_intensity_sample(const UnetrAugDesc* d, const UnetrAugIntensityDesc* it, const long long* state, int* table,
                               void* stream);
size_t unetr_aug_intensity_ws_bytes(const UnetrAugDesc* d);
int unetr_aug_intensity_apply(const UnetrAugDesc* d, const int* table, float* x, void* ws, size_t ws_bytes, void* stream);
/* Class-balanced crop centres (MONAI 0.6.0 RandCropByLabelClassesd; DESIGN.md section 12, tests/augment_classes_ref.py).
 * VolumeCache.build_class_indices: unetr_aug_class_count / _scatter build the voxel lists of map_classes_to_indices for K
 * classes (1..32) from one read of the label per pass.  L == 1: class c is lbl == c, an id >= K is in no list; L > 1 (K must be
 * L): class c is lbl[c] != 0, lists may overlap.  image_mask != 0 keeps only voxels with any_c(img > thr) (img may be NULL
 * otherwise).  count writes offsets [K + 1] (DEVICE int64: cumulative list lengths in class order; offsets[K] is the total),
 * scatter writes lists [offsets[K]] (int32): the K lists concatenated in class order, each in ascending ravel order, by a
 * stable counting sort with no atomics.  ws of unetr_aug_class_ws_ints(V, K) ints, the same for both calls.
 * unetr_aug_sample_classes is the sampler for UnetrAugDesc.sampling == 2 (which unetr_aug_sample / _affine refuse): it draws
 * what they draw, except that block 0 word 0 picks the class of the centre and word 1 the voxel of that class.  class_table is a
 * DEVICE table of int64 rows (lists ptr, offsets ptr), one per row of vols; ratios [K] is DEVICE float32, read on every call: a
 * class without voxels in the volume, or whose ratio is not a positive finite number, has weight 0; the class is the first c with
 * u * total < cum_c (double sums in class order).  With no weighted class the corner is uniform from words 0..2.  classes [B]
 * (int32) records the class drawn, -1 for the uniform corner.  a and affine are both NULL (unetr_aug_sample's draws otherwise)
 * or both given (unetr_aug_sample_affine's).  No host synchronisation.
 * (Additions: no existing signature or struct moved, UNETR_ABI_VERSION stays.) */
long unetr_aug_class_ws_ints(long V, int K);
int unetr_aug_class_count(const float* img, const unsigned char* lbl, int C, int L, int K, long V, int image_mask, float thr,
                          int* ws, size_t ws_ints, long long* offsets, void* stream);
int unetr_aug_class_scatter(const float* img, const unsigned char* lbl, int C, int L, int K, long V, int image_mask, float thr,
                            const int* ws, size_t ws_ints, const long long* offsets, int* lists, void* stream);
int unetr_aug_sample_classes(const UnetrAugDesc* d, const UnetrAugAffineDesc* a, const long long* vols, int nvol,
                             const long long* class_table, int K, const float* ratios, const int* order, long long* state,
                             int* params, float* affine, int* classes, void* stream);

/* ---- per-volume resampling and reorientation (csrc/preprocess.hip; unetr_segmentation_3d.py:326-331) ----
 * Spacingd(mode=("bilinear", "nearest")) -> Orientationd [-> ConvertToMultiChannelBasedOnBratsClassesd] as one gather: output voxel
 * (j0, j1, j2) of oimg [C,D,H,W] (float32) / olbl [L,D,H,W] (uint8) reads the source [C|L, n0, n1, n2] at
 * clamp(mat @ (j0, j1, j2, 1), 0, n - 1); mat is a HOST array of 12 doubles (3x4 row-major, preprocess.plan), evaluated in fp64 on
 * the device.  Image: float32 source, or int16 when img_int16; trilinear with fp32 weights, or one tap when every entry of mat is
 * an integer (a pure flip / transpose: values returned bit for bit).  Label: round-half-even nearest; lbl may be NULL (image
 * only); brats = 1 reads a one-channel label and writes the L = 4 channels ==0, 2|3, 1|2|3, ==3.  1 <= C, L <= 8.
 * UNETR_ERR_UNSUPPORTED for 2^31 or more source or output voxels.  No host synchronisation. */
int unetr_resample_orient(const void* img, int img_int16, const unsigned char* lbl, int C, int L, int brats, int n0, int n1, int n2,
                          const double* mat, int D, int H, int W, float* oimg, unsigned char* olbl, void* stream);

/* ---- predictions back onto a scan's own voxel grid (csrc/restore.hip) ----
 * The inverse of Spacingd -> Orientationd -> CropForegroundd as one gather (MONAI 0.6.0's Spacingd.inverse / Orientationd.inverse /
 * CropForegroundd.inverse; for BraTS the label rule of ConvertFromMultiChannelToRGB, unetr_segmentation_3d.py:95-101).  src
 * [C, crop[0], crop[1], crop[2]] (float32, or uint8 when src_u8) lives on the box origin .. origin + crop - 1 of the resampled and
 * oriented grid of extents full.  Every native voxel (i0, i1, i2) of the grid [n0, n1, n2]: s = clamp(m @ (i0, i1, i2, 1), 0,
 * full - 1) in fp64 (m: 3x4 row-major, the inverse of the forward matrix); r = rint(s), half to even; r outside the box on any
 * axis: background, every output for the voxel is 0; else nearest reads src[r - origin] and linear blends the eight taps around
 * clamp(s - origin, 0, crop - 1) with fp32 weights.  An all-integer m takes the one-tap path in every mode (bits returned).
 *   linear = 0            out = the picked voxel: float32 / uint8 [C, n0, n1, n2] (dtype of src); post must be 0
 *   linear = 1, post = 0  out = float32 [C, ...] trilinear scores (float32 src only)
 *   linear = 1, post = 1  out = uint8 [1, ...]: argmax over the C interpolated channels, first maximal channel
 *   linear = 1, post = 2  out = uint8 [C, ...]: interpolated logit >= 0
 *   brats = 1             (linear = 0, or post != 0; C = 4: background / TC / WT / ET) out = uint8 [1, ...]: 1 where WT, then 2
 *                         where TC, then 3 where ET, else 0.  A channel is set where the picked value == 1 (linear = 0), the
 *                         logit >= 0 (post = 2) or it is the argmax (post = 1).
 * 1 <= C <= 16.  The struct is passed BY VALUE; no workspace, no allocation, no host synchronisation.  UNETR_ERR_UNSUPPORTED for
 * more than 2^31 - 1 voxels on either grid or a launch-grid dimension over 65535.
 * (Additions: no existing signature moved, UNETR_ABI_VERSION stays.) */
typedef struct {
    double m[12];
    int full[3];
    int origin[3];
    int crop[3];
} unetr_restore_geom;
int unetr_restore_native(const void* src, int src_u8, int C, unetr_restore_geom g, int n0, int n1, int n2, int linear, int post,
                         int brats, void* out, void* stream);

/* ---- connected-component post-processing (csrc/postprocess.hip; monai.transforms.KeepLargestConnectedComponent of MONAI 0.6.0
 * and the min_size rule of skimage.morphology.remove_small_objects) ----
 * unetr_ccl labels the 3-D connected components of in and filters them, per *plane* of class words w (0 = not filtered):
 *   mode 0  class-id map [B,1,D,H,W] (float32, integral): one plane per item; w = id where bit id of applied is set
 *           (ids 1..31; bit 0 must be clear), w = 1 for every applied id when independent = 0;
 *   mode 1  one-hot / multi-label [B,C,D,H,W] (set where != 0): bit c of applied selects channel c; independent = 1: one plane
 *           per (item, applied channel); independent = 0: one plane per item, w = 1 where any applied channel is set;
 *   mode 2  logits [B,C,D,H,W]: first-maximum argmax (as unetr_sw_finalize_post) into out [B,1,D,H,W], then mode 0 in place.
 * Voxels are connected when they are neighbours under connectivity (1: 6, 2: 18, 3: 26) and carry the same non-zero w.  The
 * canonical label of a component is 1 + the smallest linear index (z*H + y)*W + x of its voxels.  rule 0 keeps, per (plane, w),
 * the component with the most voxels (ties: the smallest label); rule 1 keeps components of at least min_size voxels.
 * Outputs, each optional (NULL): out (layout of in; mode 2: [B,1,D,H,W], required) = in where w == 0 or the component is kept,
 * else 0; labels / sizes (int32, layout of out) = canonical label / voxel count of the voxel's component, 0 where w == 0;
 * ncomp [planes][32] (int32) = number of components per (plane, w).  Channels of mode 1 that are not applied are NOT written in
 * any output.  C <= 16; D, H, W <= 1024 and D*H*W < 2^31 - 1, else UNETR_ERR_UNSUPPORTED.  ws holds
 * unetr_ccl_workspace_bytes(D, H, W, group) bytes (0 for an unsupported shape): 9 B per voxel for each of the `group` planes
 * processed together.  Integer atomics only: results are bit-reproducible.  No host synchronisation.
 * (Additions: no existing signature moved, UNETR_ABI_VERSION stays.) */
size_t unetr_ccl_workspace_bytes(int D, int H, int W, int group);
int unetr_ccl(const float* in, float* out, int* labels, int* sizes, int* ncomp, int B, int C, int D, int H, int W, int mode,
              unsigned applied, int independent, int connectivity, int rule, int min_size, void* ws, size_t ws_bytes, int group,
              void* stream);

/* ---- binary morphology on bit-packed masks and hole filling (csrc/morphology.hip; scipy.ndimage.binary_dilation / _erosion /
 * _opening / _closing / binary_fill_holes and the fill_holes rule of MONAI) ----
 * unetr_morph treats in [B,C,D,H,W] (float32, or one byte per voxel -- uint8 / bool -- when u8) as N = B*C masks [D,H,W], set
 * where in != 0, or where in == class_id when class_id >= 0 (a class-id map), and writes 0 / 1 in the same type and layout to
 * out (which must not be in).  The masks are packed to one bit per voxel (uint64 [N,D,H,ceil(W/64)], bit b of word w = voxel
 * x = 64 w + b), stepped in that form and unpacked once:
 *   op 0  dilation: `iterations` steps with the structuring element scipy.ndimage.generate_binary_structure(3, connectivity)
 *         (connectivity 1, 2, 3 = 6, 18, 26 neighbours and the centre); every voxel outside the volume reads as border_value;
 *   op 1  erosion, likewise;
 *   op 2  opening = erosion then dilation, `iterations` steps each, border_value 0 for both (scipy.ndimage.binary_opening);
 *   op 3  closing = dilation then erosion, likewise (so it erodes at the faces of the volume, as scipy's does);
 *   op 4  contour = in & ~erosion(in, 1 step, border_value 0); iterations and border_value are not read.
 * Up to 4 steps run in one launch on tiles held in LDS, so an operation takes ceil(iterations / 4) launches besides pack and
 * unpack.  ws holds unetr_morph_workspace_bytes(D, H, W, N) bytes (0 for an unsupported shape): two packed images.
 *
 * unetr_fill_holes fills the holes of in given labels [B,C,D,H,W] (int32) = the canonical labels unetr_ccl gives the
 * components of the background in == 0 under `connectivity`.  A hole is a labelled component with no voxel on the six faces.
 *   class_map 0  N = B*C masks: out = 1 where in != 0 or the voxel lies in a hole, else 0 (scipy.ndimage.binary_fill_holes);
 *   class_map 1  class-id map [B,1,D,H,W], integral ids 0..31: a hole becomes id l when the non-zero values among the
 *                neighbours (under `connectivity`) of its voxels are all l and bit l of applied is set (bit 0 must be clear);
 *                every other voxel keeps its value.
 * ws holds unetr_fill_holes_workspace_bytes(D, H, W, N, class_map) bytes: one flag byte per voxel, and with class_map one
 * 32-bit word of neighbour ids per voxel, both addressed by canonical label and zeroed by a memset in the stream.
 *
 * Both: C <= 16; D, H, W <= 1024, D*H*W < 2^31 - 1 and B*C <= 65535, else UNETR_ERR_UNSUPPORTED.  Integer atomics only; fixed
 * grids; no allocation, no host synchronisation.  (Additions: no existing signature moved, UNETR_ABI_VERSION stays.) */
size_t unetr_morph_workspace_bytes(int D, int H, int W, int N);
int unetr_morph(const void* in, void* out, int u8, int B, int C, int D, int H, int W, int class_id, int op, int iterations,
                int connectivity, int border_value, void* ws, size_t ws_bytes, void* stream);
size_t unetr_fill_holes_workspace_bytes(int D, int H, int W, int N, int class_map);
int unetr_fill_holes(const void* in, void* out, int u8, const int* labels, int B, int C, int D, int H, int W, int class_map,
                     unsigned applied, int connectivity, void* ws, size_t ws_bytes, void* stream);

/* ---- overlap table of two label maps and the instance-level metrics on it (csrc/lesion.hip) ----
 * a, b: int32 [planes, D, H, W], 0 = not labelled, else a canonical label as unetr_ccl writes it (1 + the linear index of a
 * voxel of the same plane; any other value reads as 0).  a_mask: optional float32 [planes, D, H, W]; where it is 0 a voxel
 * still pairs its two labels but does not count towards the size of its a label or the masked count of the pair (NULL: every
 * voxel counts).  Per plane an open-addressing table of the distinct pairs (a, b) that share a voxel is built in ws:
 * slots = 2 * max_pairs rounded up to a power of two (at least 2), key (a << 32) | b with 0 = empty, slot = the 64-bit
 * MurmurHash3 finalizer of the key & (slots - 1), linear probing, value {voxels, masked voxels} (int32 each).  ws begins with
 * keys [group][slots] uint64, then (256-byte aligned) values [group][slots][2] int32; after a call with planes <= group these
 * hold the tables of all planes.  A plane with more than max_pairs distinct pairs is flagged: overflow = 1, the first five
 * values NaN and the counts that depend on the table -1.
 *   mode 0  lesion-wise: an a label i is a lesion of gv_i masked voxels; every b label p paired with it is a match;
 *           pv_i = sum of size(p) over its matches, inter_i = sum of the masked voxels of its pairs,
 *           dice_i = 2 inter_i / (pv_i + gv_i), 0 without a match; lesions with gv_i < min_size are ignored.
 *           counts = {lesions, tp, fn, fp, b labels, b labels matched to a lesion that is not ignored, overflow, distinct pairs},
 *           values = {sum dice_i, lesion Dice = sum / (tp + fn + fp) or 1 for 0/0, precision, recall, f1}.
 *   mode 1  panoptic: a pair matches when 2 n > size_a + size_b - n (IoU > 1/2, decided in integers);
 *           counts = {a labels, tp, fn, fp, b labels, tp, overflow, distinct pairs}, values = {sum IoU, sq, rq, pq}.
 * counts: int64 [planes][UNETR_LO_FIELDS], values: float64 [planes][UNETR_LO_FIELDS].  The float64 sums are taken over a fixed
 * partition in a fixed order (no float atomics): bit-reproducible.  D, H, W <= 1024, D*H*W < 2^31 - 1 and max_pairs <= 2^24,
 * else UNETR_ERR_UNSUPPORTED.  ws: 256-byte aligned, unetr_label_overlaps_workspace_bytes(D, H, W, max_pairs, group) bytes
 * (0 for an unsupported shape): 16 B per slot and 20 B per voxel for each of the `group` planes processed together.  Five
 * launches per group (the first clears the workspace); no allocation, no host synchronisation.
 * (Additions: no existing signature moved, UNETR_ABI_VERSION stays.) */
#define UNETR_LO_FIELDS 8
size_t unetr_label_overlaps_workspace_bytes(int D, int H, int W, int max_pairs, int group);
int unetr_label_overlaps(const int* a, const int* b, const float* a_mask, long planes, int D, int H, int W, int mode, int min_size,
                         int max_pairs, long long* counts, double* values, void* ws, size_t ws_bytes, int group, void* stream);

/* ---- fused AdamW over one flat fp32 buffer (torch.optim.AdamW semantics; unetr_segmentation_3d.py:522) */
int unetr_adamw(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                float eps, float weight_decay, const float* step_dev,
                void* shadow_bf16 /* optional: bf16 copy of the updated p (GEMM weight shadow), or NULL */, void* stream);

/* data-parallel form of the same update (replaces the DistributedDataParallel gradient averaging that the reference's
 * single-GPU script does not need, BASELINE.json configs[2]): g is the all-reduced SUM in the communication buffer
 * (fp32, or bf16 when g_is_bf16), gscale = 1 / world size is applied on the fly. */
int unetr_adamw_reduced(float* p, const void* g, int g_is_bf16, float gscale, float* m, float* v, long n, float lr,
                        float beta1, float beta2, float eps, float weight_decay, const float* step_dev,
                        void* shadow_bf16, void* shadow_x3 /* optional: bf16x3 word shadow of the updated p (unetr_split_words), or NULL */,
                        void* stream);

/* the streaming form that reads lr / weight_decay from a hyper row (see unetr_counter_add_lr) when the kernel runs: the argument set of
 * unetr_adamw_reduced with hyper_dev in place of (lr, weight_decay).  The same float lr gives the same bits as the by-value forms. */
int unetr_adamw_hyper(float* p, const void* g, int g_is_bf16, float gscale, float* m, float* v, long n, const float* hyper_dev,
                      float beta1, float beta2, float eps, const float* step_dev, void* shadow_bf16, void* shadow_x3, void* stream);

/* ---- gradient clipping by global L2 norm on the device (torch.nn.utils.clip_grad_norm_, error_if_nonfinite=False; grad_clip.hip) ----
 * The clip row: four floats in DEVICE memory, {norm, coef, max_norm, nonfinite}, separate from the hyper row.
 * unetr_grad_sumsq_ranges: sum of squares over n_ranges ranges of a flat gradient source (fp32, or bf16 when src_is_bf16; 16-byte
 * aligned), every element widened to double.  table (DEVICE memory, 3 longs per range, the layout of unetr_cast_bf16_ranges):
 * element offset lo, element offset hi, first block of the range in blocks of 8192 elements (running sum of ceil((hi - lo) / 8192));
 * n_blocks = total.  Only [lo, hi) is read.  Workgroup b writes its sum to partials[b] (partials_bytes >= 8 n_blocks, else
 * UNETR_ERR_WORKSPACE): no atomics, the same input gives the same bits.  unetr_grad_sumsq: one tensor of n elements at any
 * element-aligned address, ceil(n / 8192) partials.
 * unetr_grad_clip_finalize: ONE workgroup sums n_partials slots in a fixed order to S and writes the row: norm = (float)(gscale *
 * sqrt(S)) (gscale = 1 / world size for an all-reduced SUM, else 1); coef in fp32 as torch computes it, c = max_norm / (norm + 1e-6f),
 * coef = c < 1 ? c : 1, NaN for a NaN c; max_norm is READ from the row when the kernel runs (unetr_grad_clip_set: a stream-ordered
 * single-thread write, max_norm > 0, +inf = measure only), so a captured step follows a change; nonfinite += 1 when norm is inf / NaN.
 * unetr_adamw_hyper_clip: unetr_adamw_hyper with the gradient g_eff = (g * gscale) * *gcoef_dev (two fp32 roundings in that order;
 * gcoef_dev = row + 1, read when the kernel runs).  Same bits as unetr_adamw_hyper on gradients scaled that way beforehand.
 * unetr_grad_scale_ranges / unetr_grad_scale: g *= *coef_dev in place over the same table / one fp32 tensor (nothing is written
 * when the coefficient is 1).
 * (Additions: no existing signature or struct moved, UNETR_ABI_VERSION stays.) */
int unetr_grad_sumsq_ranges(const void* src_arena, int src_is_bf16, const long* table_dev, int n_ranges, long n_blocks,
                            double* partials, size_t partials_bytes, void* stream);
int unetr_grad_sumsq(const void* src, int src_is_bf16, long n, double* partials, size_t partials_bytes, void* stream);
int unetr_grad_clip_finalize(const double* partials, long n_partials, float gscale, float* clip_row, void* stream);
int unetr_grad_clip_set(float* clip_row, float max_norm, void* stream);
int unetr_adamw_hyper_clip(float* p, const void* g, int g_is_bf16, float gscale, float* m, float* v, long n, const float* hyper_dev,
                           float beta1, float beta2, float eps, const float* step_dev, void* shadow_bf16, void* shadow_x3,
                           const float* gcoef_dev, void* stream);
int unetr_grad_scale_ranges(float* grad_arena, const long* table_dev, int n_ranges, long n_blocks, const float* coef_dev, void* stream);
int unetr_grad_scale(float* g, long n, const float* coef_dev, void* stream);

/* ---- the single-GPU step's optimizer fused into the producer of the gradients (train_step.TrainStep(fuse_update=True)) ------
 * The four arenas (parameters, gradients, both moments; fp32, `total` elements, identical layout) and the optional bf16 shadow
 * arena of the parameters; steps = per-parameter step counts (float, already advanced for this step). */
typedef struct {
    float* param; const float* grad; float* m; float* v; void* shadow_bf16; const float* steps; long total;
    float lr, beta1, beta2, eps, weight_decay;
    void* shadow_x3;                  /* optional arena of bf16x3 words (unetr_split_words layout), written next to shadow_bf16; or NULL */
    const float* hyper;               /* optional hyper row in device memory: lr / weight_decay are read from it by the kernels (unetr_adamw_ranges,
                                         unetr_gemm_bf16_grouped_wgrad_adamw[_t]) instead of the by-value fields above; or NULL.
                                         (A trailing addition: a caller that zero-initialises the struct and sets the fields above keeps
                                         the by-value behaviour.  No existing signature moved, UNETR_ABI_VERSION stays -- a binding that
                                         knows this field also declares unetr_adamw_hyper, which an older library does not export.) */
} unetr_adamw_arena;
/* grouped ViT weight gradients (unetr_gemm_bf16_grouped_wgrad) whose epilogue APPLIES AdamW instead of storing dW: every
 * probs[i].dw must address a slice of a->grad (it is not written); the parameter / moment / shadow slices at the same arena
 * offset are updated with g = dW, step count a->steps[step_index[i]].  Same bits as the gradient store followed by unetr_adamw
 * (torch.nn.Linear backward + torch.optim.AdamW.step, unetr_segmentation_3d.py:224-225), 8 bytes per weight less HBM traffic. */
int unetr_gemm_bf16_grouped_wgrad_adamw(const unetr_grouped_problem* probs, int n, const unetr_adamw_arena* a,
                                        const int* step_index, void* stream);
/* the data-parallel counterpart (bf16 gradient communication, BASELINE.json configs[2]): the same grouped weight gradients stored
 * as bf16 at the arena offset of probs[i].dw (a slice of grad_arena, NOT written) in out_bf16_arena -- the communication buffer --
 * i.e. what unetr_cast_bf16 makes of the fp32 gradient, without the fp32 store, the cast pass and its re-read; and the cast of
 * every other gradient range in one launch (table in DEVICE memory, 3 longs per range: element offsets lo, hi -- multiples of
 * 8 --, first block of the range in blocks of 8192 elements, running sum; n_blocks = total). */
int unetr_gemm_bf16_grouped_wgrad_bf16out(const unetr_grouped_problem* probs, int n, const float* grad_arena, void* out_bf16_arena,
                                          long total, void* stream);
int unetr_cast_bf16_ranges(const float* src_arena, void* dst_arena, const long* table_dev, int n_ranges, long n_blocks, void* stream);
/* AdamW over n_ranges arena ranges in ONE launch (the parameters the fused launch above did not cover: biases, LayerNorm,
 * conv weights ...).  table (DEVICE memory, 4 longs per range): element offset lo, element offset hi (multiples of 4 as the
 * arena packs them), index into a->steps, first block of the range (blocks of 4096 elements, running sum); n_blocks = total. */
int unetr_adamw_ranges(const unetr_adamw_arena* a, const long* table_dev, int n_ranges, long n_blocks, void* stream);

/* ---- transposed bf16 weight shadow (bf16 mode, flat arenas): the ViT data gradients dx = dy W on the forward (b_kn = 0) kernel form ----
 * shadow_t is a second bf16 arena addressed with the element offsets of the parameter arena: a weight [N, K] at offset o has its
 * transposed twin, [K, N] row-major, at shadow_t + o.  dx[M, K] = dy[M, N] . W is then unetr_gemm_bf16 with b_kn = 0, B = shadow_t + o,
 * ldb = N (the reduction length).
 * unetr_gemm_bf16_grouped_wgrad_adamw_t: unetr_gemm_bf16_grouped_wgrad_adamw whose epilogue also writes the twin of every weight it
 * updates (whole 128-byte lines of its rows, 2 bytes per weight more than the plain form; needs a->shadow_bf16, shadow_t 16-byte
 * aligned and every probs[i].dw at an arena offset that is a multiple of 8 elements, else UNETR_ERR_UNSUPPORTED).  shadow_t == NULL runs the
 * kernel of the plain entry point; the other outputs are bit-identical either way.  Bytes of shadow_t outside the updated slices are
 * not touched.
 * unetr_transpose_bf16_grouped: the derive launch -- dst_arena + offset as [K, N] = transpose of src_arena + offset as [N, K] for every
 * table entry, in one launch (offset, N, K multiples of 8).  Used when a twin is missing or stale (first use, invalidation, optimizer
 * steps that did not go through the entry point above).
 * (Additions: no existing signature or struct moved, UNETR_ABI_VERSION stays.) */
typedef struct { long offset; int N, K; } unetr_transpose_problem;
int unetr_gemm_bf16_grouped_wgrad_adamw_t(const unetr_grouped_problem* probs, int n, const unetr_adamw_arena* a,
                                          const int* step_index, void* shadow_t, void* stream);
int unetr_transpose_bf16_grouped(const void* src_arena, void* dst_arena, const unetr_transpose_problem* probs, int n, void* stream);

/* ---- dense exact Euclidean distance transform and the distance fields (csrc/edt.hip) -----------------------
 * N = B*C binary masks [D,H,W], 1 <= C <= 16 and D, H, W <= 512 (else UNETR_ERR_UNSUPPORTED), derived from src inside the first pass:
 *   MASK       float32 [B,C,D,H,W], the mask is one where the value != 0;      MASK_U8    the same from bytes (torch.bool / uint8)
 *   CLASS_IDS  float32 class ids [B,D,H,W], the mask of channel c is one where (int)id == c
 *   SOFTMAX    float32 logits [B,C,D,H,W], one where softmax over the channels > 0.5;      SIGMOID    where sigmoid > 0.5
 * out [B,C,D,H,W] float32, every element written:
 *   DISTANCE   the distance to the nearest voxel where the mask is 0 (0 on those voxels; squared = 1: its square); +inf everywhere
 *              for a mask without a zero
 *   SIGNED     d_fg outside the object, -(d_bg - u) inside it; d_fg / d_bg = the distance to the nearest voxel where the mask is
 *              one / zero, u = 1 without a spacing, else the smallest spacing
 *   UNSIGNED   (d_fg + d_bg)^alpha, alpha > 0; accumulate = 1 adds it to what out holds
 *   SIGNED and UNSIGNED are 0 everywhere for a mask that is empty or fills the volume.
 * spacing[3] = (z, y, x) voxel size when has_spacing, else 1.  float32 arithmetic: every term (s k)^2 with two roundings, the sum
 * as (x + y) + z; exact integers without a spacing.
 * ws: 16-byte aligned.  unetr_edt_workspace_bytes = what runs all B items in one group of three launches (0 for a descriptor that
 * is refused); any ws that holds one item's share (that / B) is accepted and the items then run in groups.  Launches on one
 * stream only: no allocation, no host synchronisation.
 * (Additions: no existing signature moved, UNETR_ABI_VERSION stays.) */
enum { UNETR_EDT_FORM_MASK = 0, UNETR_EDT_FORM_MASK_U8 = 1, UNETR_EDT_FORM_CLASS_IDS = 2, UNETR_EDT_FORM_SOFTMAX = 3,
       UNETR_EDT_FORM_SIGMOID = 4 };
enum { UNETR_EDT_FIELD_DISTANCE = 0, UNETR_EDT_FIELD_SIGNED = 1, UNETR_EDT_FIELD_UNSIGNED = 2 };
typedef struct unetr_edt_desc {
    int B, C, D, H, W;
    int form, field, squared, accumulate, has_spacing;
    float spacing[3];
    float alpha;
} unetr_edt_desc;
size_t unetr_edt_workspace_bytes(const unetr_edt_desc* d);
int unetr_edt(const unetr_edt_desc* d, const void* src, float* out, void* ws, size_t ws_bytes, void* stream);

/* ---- distance-map losses (csrc/dist_loss.hip) on logits [B,C,V] fp32, 1 <= C <= 16 -------------------------
 * multilabel = 0: target [B,V] float class ids, p = softmax over the channels; multilabel = 1: target [B,C,V] float mask, p = sigmoid.
 *   BOUNDARY   out[0] = *weight * mean over (b, included c, v) of p * field            (field = the SIGNED field of the target;
 *                                                                                        target itself is not read and may be NULL)
 *   HAUSDORFF  out[0] = *weight * mean over (b, included c, v) of (p - g)^2 * field    (field = UNSIGNED^alpha of the prediction
 *                                                                                        mask + that of the target; no gradient)
 * The mean runs over all channels, or 1..C-1 with include_background = 0 (C >= 2); an excluded channel still takes part in the
 * softmax.  weight: one float32 in device memory, read when the kernels run.  ws: 16-byte aligned, unetr_distloss_workspace_bytes.
 * Fixed-order partial sums, finalized by one block in double: reproducible run to run, no float atomics.
 * unetr_distloss_bwd: dlogits = *dloss (device scalar; NULL = 1) * dout[0]/dlogits, every element written.
 * Launches only: no allocation, no host synchronisation.  (Additions: no existing signature moved, UNETR_ABI_VERSION stays.) */
enum { UNETR_DISTLOSS_BOUNDARY = 0, UNETR_DISTLOSS_HAUSDORFF = 1 };
typedef struct unetr_distloss_desc {
    int B, C;
    long V;
    int multilabel, kind, include_background;
} unetr_distloss_desc;
size_t unetr_distloss_workspace_bytes(const unetr_distloss_desc* d);
int unetr_distloss_fwd(const unetr_distloss_desc* d, const float* logits, const float* target, const float* field,
                       const float* weight, float* out, void* ws, size_t ws_bytes, void* stream);
int unetr_distloss_bwd(const unetr_distloss_desc* d, const float* logits, const float* target, const float* field,
                       const float* weight, const float* dloss, float* dlogits, void* stream);

/* ---- exact order statistic of an fp32 array (csrc/select.hip): a radix select over the bit pattern -----------
 * x[n] fp32, contiguous, 1 <= n < 2^31 (else UNETR_ERR_UNSUPPORTED), any alignment (16-byte loads when n % 4 == 0 and x is 16-byte
 * aligned, one element per thread otherwise).  The 0-based rank r is read from device memory (*rank, clamped to [0, n-1]) WHEN THE
 * KERNELS RUN; rank == NULL takes rank_host (0 <= rank_host < n) instead.  flags: UNETR_SELECT_LARGEST = r-th largest, else r-th
 * smallest; UNETR_SELECT_PLAIN_HIST = the first histogram pass without its LDS-contention remedy (a measurement switch, same result).
 * Order: the keys  bits ^ (sign ? 0xFFFFFFFF : 0x80000000)  as unsigned integers -- negatives, -0 < +0, denormals and +-inf are all
 * ordered, NaNs sort at the two ends.
 * out (device memory): value = the element of that rank; n_beyond = elements strictly beyond it on the selected side (greater for
 * LARGEST, smaller otherwise); n_equal = elements with the same bits.
 * Six launches on `stream` -- init, four 8-bit histogram passes (each picks its predecessor's digit in its prologue), final pick --
 * with integer counts only: bitwise reproducible; no allocation, no host synchronisation, no data-dependent loop, no hand-off
 * between workgroups inside a kernel.  ws: 16-byte aligned, unetr_select_workspace_bytes(n) = (4*256 + 16) * 4 = 4160 bytes (0 for an
 * n that is refused); the init launch zeroes every histogram word that is read, so the scratch may hold anything.
 * (Additions: no existing signature moved, UNETR_ABI_VERSION stays.) */
enum { UNETR_SELECT_LARGEST = 1, UNETR_SELECT_PLAIN_HIST = 2 };
typedef struct unetr_select_result {
    float value;
    unsigned n_beyond, n_equal;
} unetr_select_result;
size_t unetr_select_workspace_bytes(long n);
int unetr_select_kth(const float* x, long n, const int* rank, int rank_host, int flags, unetr_select_result* out, void* ws,
                     size_t ws_bytes, void* stream);

/* ---- top-k cross entropy (csrc/topk_loss.hip) on logits [B,C,V] fp32, 1 <= C <= 16 and B*V < 2^31 (else UNETR_ERR_UNSUPPORTED) ---
 * multilabel = 0: label [B,V] float class ids; multilabel = 1: mask [B,C,V], the class of a voxel is the FIRST argmax of its mask
 * (as seg_loss.hip).  Per-voxel value  u_v = w[y_v] * (logf(sum_c e^(z_c - max)) - (z_y - max)),  w = class_weight [C] (non-negative,
 * device memory, multilabel = 0 only) or NULL = 1; with has_ignore (multilabel = 0 only) a voxel labelled ignore_index has no value
 * and no gradient.
 *   N = number of voxels with a value over the WHOLE batch (all B*V),  K = max(1, floor((double)N * (double)*k / 100.0)),
 *   k = a percentage in (0, 100], one float32 in device memory, read when the kernels run (N and K are computed on the device);
 *   t = the K-th largest value, n_gt = #{u > t}, n_eq = #{u == t};
 *   X = (sum_{u > t} u + (K - n_gt) * t) / K    (= torch.topk(u, K).values.mean()), summed in a fixed order, finalized in double;
 *   dX/du_v = 1/K where u > t, (K - n_gt) / (n_eq * K) where u == t, 0 elsewhere: ties at the threshold share the remaining weight
 *   equally (deterministic, no indices; differs from topk's arbitrary pick only on exact ties).
 * unetr_topkce_fwd: values [B*V] floats receives u (an ignored voxel: -1) and is kept for backward together with coef [4] =
 *   {1/K, (K - n_gt)/(n_eq K), t, 0}; out [4] = {X, t, K, N}.  Ten launches: values, rank, the six of unetr_select_kth, sum, final.
 *   ws: 16-byte aligned, unetr_topkce_workspace_bytes = 4160 (the select's) + 32 + 4 * B * ceil(V / 1024) + 4 * ceil(B*V / 4096),
 *   rounded up to a multiple of 16 (0 for a descriptor that is refused).
 * unetr_topkce_bwd: dlogits = *dloss (device scalar; NULL = 1) * dX/du_v * w_y * (softmax - onehot), every element written; it
 *   compares the bits of `values` with t, never a recomputed value.
 * Launches only: no allocation, no host synchronisation, no float atomics.  (Additions: no existing signature moved,
 * UNETR_ABI_VERSION stays.) */
typedef struct unetr_topkce_desc {
    int B, C;
    long V;
    int multilabel, has_ignore, ignore_index;
    const float* class_weight;
} unetr_topkce_desc;
size_t unetr_topkce_workspace_bytes(const unetr_topkce_desc* d);
int unetr_topkce_fwd(const unetr_topkce_desc* d, const float* logits, const float* label, const float* k, float* values, float* out,
                     float* coef, void* ws, size_t ws_bytes, void* stream);
int unetr_topkce_bwd(const unetr_topkce_desc* d, const float* logits, const float* label, const float* values, const float* coef,
                     const float* dloss, float* dlogits, void* stream);

#ifdef __cplusplus
}
#endif
#endif
