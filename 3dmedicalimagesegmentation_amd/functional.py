"""Host-side composition of the HIP kernels into differentiable blocks (torch.autograd.Function).

PyTorch is plumbing here: it owns device memory (caching allocator), streams and the autograd graph; every
FLOP of the hot path runs in libunetr_hip.so through the C ABI of include/unetr_hip.h.  Tensors that reach
these functions must live on a ROCm device -- there is no CPU or eager-PyTorch fallback.

Layouts: token matrices [B*L, H]; feature maps channels-last [B, D, H, W, C] (possibly row-pitched views).
"""
import collections
import ctypes
import os

import torch

from . import _capi, derived_weights, grad_arena
from ._capi import GemmDesc, GemmBf16Desc, call, call_rc
from .derived_weights import (_split_words, after_step, conv_pack_get, drop_wt_shadow, invalidate_weight_shadows,  # noqa: F401
                              records_of, refresh_conv_packs, refresh_derived_weights, register_weight_shadow, shadow_at,
                              shadow_ptr_for_update, twin_at, weight_bf16, weight_bf16_t, weight_x3, wt_enabled)
from .grad_arena import (ArenaState, _DEFAULT_STATE, _gout, _ret, clear_grad_sinks, flush_deferred,  # noqa: F401
                         register_grad_sinks)

LN_EPS = 1e-5
IN_EPS = 1e-5

_WS = {}
_WS_BYTES = int(os.environ.get("UNETR_AMD_WS_MB", "256")) << 20     # largest users: split-K slabs (M x N x splits fp32), InstanceNorm
                                                                     # partial rows, weight-gradient partials outside arena mode
_WS_SHARED = {}                                                      # device index -> stream ids that use the device's shared buffer


def share_workspace(stream):
    """Declare that work on `stream` never runs concurrently with work on the device's default stream or on another stream declared
    here -- the caller orders them with wait_stream / graph-replay order (train_step.side_stream: eager warm-up and graph capture
    run there while the launching stream waits; replays are launched on the launching stream).  Such streams use ONE scratch buffer
    per device instead of one each (256 MB per (device, stream) before: main + warm-up + capture = 768 MB)."""
    _WS_SHARED.setdefault(stream.device.index, set()).add(stream.cuda_stream)


def workspace(device):
    """Scratch for split-K slabs and reduction partials: one buffer per (device, stream) -- reuse inside a stream is
    stream-ordered and therefore safe; two streams (e.g. two models stepping concurrently) never share one -- except the streams
    declared by share_workspace, which together with the default stream share the device's buffer."""
    sid = torch.cuda.current_stream(device).cuda_stream
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if sid == 0 or sid in _WS_SHARED.get(idx, ()):
        sid = 0
    key = (device.type, idx, sid)
    ws = _WS.get(key)
    if ws is None:
        ws = torch.empty(_WS_BYTES // 4, dtype=torch.float32, device=device)
        _WS[key] = ws
    return ws


def release_workspaces():
    """drop every scratch buffer (they are re-created on demand; captured graphs that baked a pointer must be dropped first)"""
    _WS.clear()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- arena gradients (grad_arena.py): where a parameter's gradient goes, and the work deferred to the end of backward ----
# In arena mode the Linear weight / bias gradients of the ViT are not needed by anything inside backward, so they are queued on
# the model's ArenaState and executed at the end of the backward pass as ONE grouped GEMM launch + ONE grouped column-sum launch
# (csrc: gemm_grouped_wgrad_kernel, colsum_grouped_kernel) instead of ~90 small latency-bound launches.
def wgrad_or_defer(dy, x, prec, w, dyb=None, xb=None):
    """dw[N,K] = dy^T x for Linear weight `w`; returns (grad_or_None_for_autograd).  dyb / xb: bf16 twins of dy / x -- the
    deferred launch then runs the bf16-storage grouped kernel (unetr_gemm_bf16_grouped_wgrad)."""
    st, out = grad_arena.dest(w)
    twins = dyb is not None and xb is not None and dyb.shape[0] % 8 == 0 and dyb.shape[1] % 8 == 0 and xb.shape[1] % 8 == 0
    if st is None:
        if not twins:
            return linear_wgrad(dy, x, prec)
        dw = torch.empty(dyb.shape[1], xb.shape[1], dtype=torch.float32, device=dyb.device)
        grad_arena.launch_wgrad_bf16([(dyb, xb, dw)])
        return dw
    if twins:
        st.queue_wgrad_bf16(dyb, xb, out)
    else:
        st.queue_wgrad(dy, x, out, prec)
    return _ret(w, out, deferred=True)


def colsum_or_defer(x, M, N, ld, b, view_shape=None):
    st, out = grad_arena.dest(b)
    if st is None:
        if x.dtype == torch.bfloat16:          # (bf16 rows: the grouped kernel reads them; one problem, launched now)
            r = torch.empty(N, dtype=torch.float32, device=x.device)
            grad_arena.launch_colsums([(x, r, M, N, ld)])
        else:
            r = colsum(x, M, N, ld)
        return r.view(view_shape) if view_shape is not None else r
    st.queue_colsum(x, out, M, N, ld)
    return _ret(b, out, deferred=True)


def act_dtype(prec):
    """storage type of the conv side's feature maps and their gradients: bf16 in bf16 precision mode (half the HBM bytes of
    the bandwidth-bound InstanceNorm / conv passes), fp32 in fp32 mode.  The C ABI infers it from `prec` (csrc/common.hpp)."""
    return torch.bfloat16 if prec == _capi.PREC_BF16 else torch.float32


def _a16(t):
    return int(t.dtype == torch.bfloat16)


def _prec_of(t):
    return _capi.PREC_BF16 if t.dtype == torch.bfloat16 else _capi.PREC_F32


def _as_act(t, prec):
    """tensor in the activation storage type of `prec` (a torch cast: only on the rare generic-fallback boundaries)"""
    dt = act_dtype(prec)
    return t if t.dtype == dt else t.to(dt)


# The generic GEMM families (im2col conv, transposed conv, unetr_gemm) read and write fp32 storage only.  Where a bf16-stored tensor
# meets them -- shapes the dedicated kernels decline -- these two casts are the boundary: exact on the way in, the activation
# storage's own rounding on the way back.
def _f32_rows(t, ld, c):
    """(fp32 rows, their pitch) of the first `c` channels of a tensor with row pitch `ld`: the tensor itself when it is fp32"""
    if t.dtype == torch.float32:
        return t, ld
    if ld != c:
        t = t[..., :c]
    return t.float().contiguous(), c


def _act_rows(t32, prec, out=None):
    """the way back: fp32 rows into the activation storage of `prec` -- a new tensor, or `out` (any row pitch)"""
    if out is None:
        return _as_act(t32, prec)
    out.copy_(t32)
    return out


def _require_gpu(t, act=False, ids=False):
    if not t.is_cuda:
        raise RuntimeError("3dmedicalimagesegmentation_amd: the HIP backend needs tensors on a ROCm device "
                           "(got a CPU tensor); there is no CPU fallback.")
    if t.dtype != torch.float32 and not (act and t.dtype == torch.bfloat16) and not (ids and t.dtype == torch.uint8):
        raise RuntimeError(f"3dmedicalimagesegmentation_amd: fp32 storage expected, got {t.dtype}")
    if t.device.index != torch.cuda.current_device():
        # kernels are launched on the CURRENT device's stream with raw pointers: a tensor of another GPU would fault
        raise RuntimeError(f"3dmedicalimagesegmentation_amd: tensor lives on {t.device} but the current device is "
                           f"cuda:{torch.cuda.current_device()}; call torch.cuda.set_device({t.device.index}) (one process per GPU)")


def _rows(t):
    """(tensor, ld) for a tensor usable as a row-pitched matrix [rows, C]: last dim contiguous and all
    leading dims collapsible with a single pitch.  Falls back to a contiguous copy."""
    c = t.shape[-1]
    if t.stride(-1) == 1 and t.dim() >= 2:
        ld = t.stride(-2)
        al = 16 // t.element_size()            # elements per 16 bytes
        ok = ld >= c and (ld % al == 0 or (ld == c and t.dtype == torch.float32)) and t.data_ptr() % 16 == 0
        exp = ld
        for d in range(t.dim() - 2, -1, -1):
            if t.shape[d] != 1 and t.stride(d) != exp:
                ok = False
                break
            exp *= t.shape[d]
        if ok:
            return t, ld
    t = t.contiguous()
    return t, c


# ------------------------------------------------------------------------------------------------ wrappers
def _p(t):
    return t.data_ptr() if t is not None else None


def _epilogue(d, bias=None, res=None, ldr=0, res_mod=0, pre=None, aux=None, ldaux=0, act=0, accumulate=False, alpha=1.0):
    """the epilogue fields that GemmDesc and GemmBf16Desc share"""
    d.bias, d.res, d.ldr, d.res_mod = _p(bias), _p(res), ldr, res_mod
    d.pre, d.aux, d.ldaux = _p(pre), _p(aux), ldaux
    d.act, d.accumulate, d.alpha = act, int(accumulate), alpha
    return d


def gemm(A, B, C, M, N, K, *, lda, ldb, ldc, prec, a_trans=False, b_trans=False, bias=None, res=None, ldr=0,
         res_mod=0, pre=None, aux=None, ldaux=0, act=0, accumulate=False, alpha=1.0, b_words=None):
    """b_words (bf16x3 mode): the pre-split word shadow of the weight B (weight_x3) -- read instead of B where the LDS-DMA kernel takes
    the shape (M >= 32, K % 32 == 0, N % 4 == 0, plain row pitches)"""
    d = _epilogue(GemmDesc(), bias, res, ldr, res_mod, pre, aux, ldaux, act, accumulate, alpha)
    d.b_x3words = 0
    if (b_words is not None and prec == _capi.PREC_BF16X3 and not a_trans and M >= 32 and K % 32 == 0 and N % 4 == 0 and lda % 4 == 0
            and ldb % 4 == 0 and ldc % 4 == 0 and (not b_trans or N >= 64)):
        B = b_words
        d.b_x3words = 1
    d.M, d.N, d.K, d.batch = M, N, K, 1
    d.a_trans, d.b_trans = int(a_trans), int(b_trans)
    d.lda, d.ldb, d.ldc = lda, ldb, ldc
    d.strideA = d.strideB = d.strideC = d.strideR = 0
    d.prec = prec
    ws = workspace(C.device)
    call("unetr_gemm", ctypes.byref(d), A.data_ptr(), B.data_ptr(), C.data_ptr(), ws.data_ptr(), ws.numel() * 4, _stream())


def cast_bf16(src, out=None):
    """fp32 -> bf16 (RNE) copy through the HIP cast kernel"""
    src = src.contiguous()
    if out is None:
        out = torch.empty(src.shape, dtype=torch.bfloat16, device=src.device)
    call("unetr_cast_bf16", src.data_ptr(), out.data_ptr(), src.numel(), _stream())
    return out


def gemm_bf16(A, B, M, N, K, *, b_kn=False, C=None, Cb=None, lda=None, ldb=None, bias=None, res=None, ldr=0, res_mod=0,
              pre=None, aux=None, ldaux=0, act=0, accumulate=False, alpha=1.0, ldcb=None, tc=None):
    """C / Cb [M,N] = epilogue(A[M,K] @ (B[N,K]^T | B[K,N])) with bf16-stored operands (csrc/gemm_bf16.hip)"""
    assert A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16
    d = _epilogue(GemmBf16Desc(), bias, res, ldr, res_mod, pre, aux, ldaux, act, accumulate, alpha)
    d.M, d.N, d.K, d.b_kn = M, N, K, int(b_kn)
    d.lda = lda if lda is not None else K
    d.ldb = ldb if ldb is not None else (N if b_kn else K)
    d.ldc = d.ldcb = N
    if ldcb is not None:
        d.ldcb = ldcb
    if tc is not None:              # (D, H, W, Cout): scatter the bf16 output as a 2x2x2 transposed conv (tap-major columns)
        d.tc_d, d.tc_h, d.tc_w, d.tc_cout = tc
    ws = workspace(A.device)
    call("unetr_gemm_bf16", ctypes.byref(d), A.data_ptr(), B.data_ptr(), _p(C), _p(Cb), ws.data_ptr(), ws.numel() * 4, _stream())


# ---- derived weight copies: derived_weights.py owns the tables and the freshness rules; the ops read weights through its getters ----
grad_arena._stream = derived_weights._stream = _stream


def begin_forward(state=None):
    """Called by UNETR.forward: a new pass starts a new weight epoch, and what a failed step left behind is dropped -- deferred
    weight-gradient work, and a fused epilogue (AdamW.begin_fused_step / TrainStep's bf16 communication form) armed for it."""
    derived_weights.begin_forward()
    if state is not None:
        state.reset_deferred()
        state.fuse = None          # an optimizer / communication epilogue is armed AFTER the forward of the step it belongs to:
                                   # whatever a failed step left armed must not ride on the next backward


# Prefetch riders: the launch just before a ViT Linear GEMM (a LayerNorm, the attention core) carries spare workgroups that read
# the bf16 weights of the GEMM(s) behind it into the Infinity Cache (include/unetr_hip.h: unetr_prefetch).  Results are
# bit-identical with and without; False launches every host exactly as without riders (tests/test_prefetch_rider_gpu.py), a
# collection of host names ("attn_fwd", "ln1_fwd", "ln2_fwd", "ln1_bwd", "ln2_bwd", "attn_bwd") keeps only those (per-host A/B).
PREFETCH_RIDERS = True


def _prefetch(host, *weights, dgrad=0):
    """unetr_prefetch over the bf16 shadows of up to two weights for the launch `host`, or None.  Only a shadow that already
    exists is named (its buffer lives as long as the parameter and is what the GEMM itself reads): no cast is launched from here.
    dgrad (token rows of the pass, or 0): the GEMM behind the launch is a data gradient -- it reads the transposed twin where
    _dgrad_operand will hand one out (a current one, M <= WT_MAX_ROWS, and under capture only to a pass that rewrites it)."""
    if not PREFETCH_RIDERS or (PREFETCH_RIDERS is not True and host not in PREFETCH_RIDERS):
        return None
    pf, n = _capi.Prefetch(), 0
    for w in weights:
        if w is None:
            continue
        # (by storage address: callers hand detached aliases of the next / lower block's parameters)
        buf = twin_at(w) if dgrad and wt_enabled() and dgrad <= WT_MAX_ROWS else None
        if buf is None:
            buf = shadow_at(w)
        if buf is not None:
            pf.ptr[n], pf.bytes[n] = buf.data_ptr(), buf.numel() * 2
            n += 1
    return pf if n else None


def _bf16_path(prec, *kdims):
    return prec == _capi.PREC_BF16 and all(k % 64 == 0 for k in kdims)


def _twin(t):
    """bf16 copy of an fp32 activation / gradient: the twin its producer attached, else a cast"""
    if t.dtype == torch.bfloat16:
        return t
    tw = getattr(t, "_unetr_bf16", None)
    if tw is not None and tw[0].numel() == t.numel() and tw[1] == t._version and t.is_contiguous():   # autograd may accumulate into t in place
        return tw[0].view(t.shape)
    return cast_bf16(t)


def _attach_twin(t, tb):
    t._unetr_bf16 = (tb, t._version)


def carry_twin(src, dst):
    """dst is the same values as src under another tensor object (a detached leaf, an alias returned by a Function): the bf16
    twin and the stashed LayerNorm of src describe dst too"""
    tw = getattr(src, "_unetr_bf16", None)
    if tw is not None and tw[1] == src._version:
        dst._unetr_bf16 = (tw[0], dst._version)
    return _carry_ln(src, dst)


def _carry_ln(src, dst):
    """the stashed LayerNorm alone (TransformerBlockFn.forward's contiguous copy of its input: nothing reads a bf16 twin of it)"""
    if dst is not src and hasattr(src, "_unetr_ln"):
        dst._unetr_ln = src._unetr_ln
    return dst


def add_cast(a, b, want_bf16=True):
    """a + b (fp32) and its bf16 twin in one launch (csrc: add_cast_bf16_kernel)"""
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty_like(a)
    ok16 = want_bf16 and a.numel() % 4 == 0
    ob = torch.empty(a.shape, dtype=torch.bfloat16, device=a.device) if ok16 else None
    if a.numel() % 4 or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise RuntimeError("add_cast needs fp32 tensors with a multiple of 4 elements")
    call("unetr_add_cast_bf16", a.data_ptr(), b.data_ptr(), out.data_ptr(), _p(ob), a.numel(), _stream())
    if ob is not None:
        _attach_twin(out, ob)
    return out


class TapFn(torch.autograd.Function):
    """A hidden state with TWO consumers (unetr.py:197-201: z3 / z6 / z9 feed the next transformer block and encoder2-4):
    forward hands out two aliases, backward sums the two gradients AND forms the bf16 operand of the producing block's backward
    GEMMs in one HIP launch -- autograd's own fan-in was an elementwise add kernel, and the twin-less sum then cost a cast."""

    @staticmethod
    def forward(ctx, x, want_bf16):
        ctx.want_bf16 = bool(want_bf16)
        a, b = x.view_as(x), x.view_as(x)
        carry_twin(x, a)
        carry_twin(x, b)
        return a, b

    @staticmethod
    def backward(ctx, ga, gb):
        if ga is None or gb is None:
            return (ga if gb is None else gb), None
        _require_gpu(ga)
        return add_cast(ga, gb, ctx.want_bf16), None


def linear_fwd(x, w, bias, prec, res=None, res_mod=0, act=0, pre=None):
    """y[M,N] = act(x[M,K] @ w[N,K]^T + bias) + res"""
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty(M, N, dtype=torch.float32, device=x.device)
    gemm(x, w, y, M, N, K, lda=K, ldb=K, ldc=N, prec=prec, bias=bias, res=res, ldr=N, res_mod=res_mod, act=act, pre=pre,
         b_words=weight_x3(w) if prec == _capi.PREC_BF16X3 else None)
    return y


def linear_dgrad(dy, w, prec, aux=None):
    """dx[M,K] = dy[M,N] @ w[N,K]  (optionally times gelu'(aux))"""
    M, N = dy.shape
    K = w.shape[1]
    dx = torch.empty(M, K, dtype=torch.float32, device=dy.device)
    gemm(dy, w, dx, M, K, N, lda=N, ldb=K, ldc=K, prec=prec, b_trans=True, aux=aux, ldaux=K, act=2 if aux is not None else 0,
         b_words=weight_x3(w) if prec == _capi.PREC_BF16X3 else None)
    return dx


def linear_wgrad(dy, x, prec, out=None):
    """dw[N,K] = dy[M,N]^T @ x[M,K]"""
    M, N = dy.shape
    K = x.shape[1]
    dw = out if out is not None else torch.empty(N, K, dtype=torch.float32, device=dy.device)
    gemm(dy, x, dw, N, K, M, lda=N, ldb=K, ldc=K, prec=prec, a_trans=True, b_trans=True)
    return dw


def colsum(x, M, N, ld, out=None):
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=x.device)
    ws = workspace(x.device)
    call("unetr_colsum", x.data_ptr(), ld, M, N, out.data_ptr(), 0, ws.data_ptr(), ws.numel() * 4, _stream())
    return out


def bf16_like(t):
    return torch.empty(t.shape, dtype=torch.bfloat16, device=t.device)


def layernorm_fwd(x, w, b, bf16_out=None, want_fp32=True, pf=None):
    M, H = x.shape
    y = torch.empty_like(x) if want_fp32 else None
    mean = torch.empty(M, dtype=torch.float32, device=x.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x.device)
    call("unetr_layernorm_fwd_pf", x.data_ptr(), w.data_ptr(), b.data_ptr(), _p(y), _p(bf16_out), mean.data_ptr(),
         rstd.data_ptr(), M, H, LN_EPS, _stream(), pf)
    return y, mean, rstd


def layernorm_bwd(dy, x, w, mean, rstd, dres=None, out_w=None, out_b=None, dx_bf16=None, pf=None, part=None):
    """part: a private buffer [ceil(M / 4), 2H] -- the kernel leaves its dgamma | dbeta partials per row block there and writes no
    dw / db (returned as None); without it the partials go through the workspace and are reduced into dw / db"""
    M, H = x.shape
    dx = torch.empty_like(x)
    dw = db = None
    if part is None:
        dw = out_w if out_w is not None else torch.empty(H, dtype=torch.float32, device=x.device)
        db = out_b if out_b is not None else torch.empty(H, dtype=torch.float32, device=x.device)
    buf = part if part is not None else workspace(x.device)
    call("unetr_layernorm_bwd_pf", dy.data_ptr(), x.data_ptr(), w.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
         _p(dx_bf16), _p(dres), _p(dw), _p(db), M, H, buf.data_ptr(), buf.numel() * 4, _stream(), pf)
    return dx, dw, db


def _ln_param_grads(w, b, M, H, device, kernel):
    """What the two LayerNorm backward forms share: (dx, grad_w, grad_b) as autograd wants them from ``kernel(dw, db, part) -> dx``.
    In arena mode the dgamma/dbeta reduction over row blocks is not needed inside backward: the kernel is handed a private buffer
    `part` for its partials (and no dw / db) and the two column sums over the halves of that buffer join the grouped launch at the
    end of the pass (one launch for all 25 LayerNorms).  Otherwise it reduces into dw / db itself (part is None)."""
    st, (ow, ob) = grad_arena.dests(w, b)
    if st is None:
        dw = ow if ow is not None else torch.empty(H, dtype=torch.float32, device=device)
        db = ob if ob is not None else torch.empty(H, dtype=torch.float32, device=device)
        return kernel(dw, db, None), _ret(w, dw), _ret(b, db)
    nblk = (M + 3) // 4
    part = torch.empty(nblk * 2 * H, dtype=torch.float32, device=device)
    dx = kernel(None, None, part)
    st.queue_colsum(part, ow, nblk, H, 2 * H)
    st.queue_colsum(part[H:], ob, nblk, H, 2 * H)
    return dx, _ret(w, ow, deferred=True), _ret(b, ob, deferred=True)


def layernorm_bwd_params(dy, x, w, b, mean, rstd, dres=None, dx_bf16=None, pf=None):
    """LayerNorm backward returning (dx, grad_w, grad_b) as autograd wants them"""
    M, H = x.shape
    return _ln_param_grads(w, b, M, H, x.device, lambda dw, db, part: layernorm_bwd(
        dy, x, w, mean, rstd, dres=dres, out_w=dw, out_b=db, dx_bf16=dx_bf16, pf=pf, part=part)[0])


def x3_ride_ok(M, N, K):
    """shapes the bf16x3 LDS-DMA GEMM takes (csrc/gemm_bf16.hip: unetr_gemm_x3_dma) -- where the LayerNorm-riding forms can be used"""
    return M >= 32 and K % 32 == 0 and N % 4 == 0 and N >= 64 and os.environ.get("UNETR_X3_GEMM_DMA", "1") != "0"


def gemm_bf16_ln_fwd(A, B, M, N, K, C, gamma, beta, y_bf16, bias=None, res=None, ldr=0, y=None, b_words=None, pf=None):
    """C[M,N] = A[M,K] @ B[N,K]^T + bias + res, and y_bf16 = LayerNorm(C) (gamma, beta) with its (mean, rstd):
    unetr_gemm_bf16_ln_fwd -- the LayerNorm of the NEXT layer rides on the split-K reduction of this GEMM.
    bf16x3 mode: A / B fp32 (B optionally as its word shadow b_words), the normalised rows go to the fp32 tensor ``y``."""
    x3 = A.dtype == torch.float32
    assert x3 or (A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16)
    d = _epilogue(GemmBf16Desc(), bias, res, ldr)
    d.x3 = (2 if b_words is not None else 1) if x3 else 0
    if b_words is not None:
        B = b_words
    d.M, d.N, d.K, d.b_kn = M, N, K, 0
    d.lda, d.ldb, d.ldc, d.ldcb = K, K, N, N
    mean = torch.empty(M, dtype=torch.float32, device=C.device)
    rstd = torch.empty(M, dtype=torch.float32, device=C.device)
    ws = workspace(C.device)
    call("unetr_gemm_bf16_ln_fwd_pf", ctypes.byref(d), A.data_ptr(), B.data_ptr(), C.data_ptr(), gamma.data_ptr(), beta.data_ptr(), LN_EPS,
         _p(y), _p(y_bf16), mean.data_ptr(), rstd.data_ptr(), ws.data_ptr(), ws.numel() * 4, _stream(), pf)
    return mean, rstd


def ln_ride_enabled():
    """norm1 of block i+1 is formed by the kernel that sums block i's last split-K GEMM (unetr_gemm_bf16_ln_fwd) instead of
    its own launch: bit-identical and one launch less per block.  On by default since round 3 (4.527 vs 4.544 ms/step in three
    interleaved rounds on one box) -- it had measured neutral while the LayerNorm kernel walked the slabs in a run-time loop, one
    memory round trip per slab and vector; with every load of the row requested up front the row-owning form wins.
    UNETR_AMD_LN_RIDE=0 restores the separate split-K reduce + LayerNorm launches.  The backward counterpart
    (unetr_gemm_bf16_ln_bwd) is always on."""
    return os.environ.get("UNETR_AMD_LN_RIDE", "1") == "1"


def _stash_ln(x, gamma, beta, xn, mean, rstd):
    """remember on the residual-stream tensor x that LayerNorm(x; gamma, beta) already exists (computed by the kernel that
    produced x): the consumer that would launch exactly that LayerNorm takes it from here (_stashed_ln)"""
    x._unetr_ln = (xn, mean, rstd, gamma.data_ptr(), gamma._version, beta.data_ptr(), beta._version, x._version)


def _stashed_ln(x, gamma, beta):
    st = getattr(x, "_unetr_ln", None)
    if st is None or st[3:] != (gamma.data_ptr(), gamma._version, beta.data_ptr(), beta._version, x._version) or st[0].shape != x.shape:
        return None
    return st[0], st[1], st[2]


def gemm_ln_bwd_params(A, Bw, M, N, K, x, w, b, mean, rstd, dres=None, dx_bf16=None, b_words=None, pf=None, b_kn=True):
    """(dx, grad_w, grad_b) of a LayerNorm whose output gradient is dy = A[M,K] @ Bw[K,N] (the data gradient of the Linear
    layer behind it, bf16-stored operands, Bw read as the [K, N] operand): unetr_gemm_bf16_ln_bwd -- when the GEMM is cut into K
    slabs the LayerNorm kernel sums them itself, so the separate split-K reduce launch disappears (bit-identical).
    b_kn=False: Bw is the transposed twin [N, K] of the weight (weight_bf16_t), read in the forward kernel form."""
    x3 = A.dtype == torch.float32              # bf16x3 mode: fp32 operands (Bw optionally as its word shadow b_words)
    assert x3 or (A.dtype == torch.bfloat16 and Bw.dtype == torch.bfloat16)
    d = _epilogue(GemmBf16Desc())
    d.x3 = (2 if b_words is not None else 1) if x3 else 0
    if b_words is not None:
        Bw = b_words
    d.M, d.N, d.K, d.b_kn = M, N, K, int(bool(b_kn))
    d.lda, d.ldb, d.ldc, d.ldcb = K, (N if b_kn else K), N, N
    scratch = torch.empty(M, N, dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    ws = workspace(x.device)

    def kernel(dw, db, part):
        lnws = part if part is not None else torch.empty((M + 3) // 4 * 2 * N, dtype=torch.float32, device=x.device)
        call("unetr_gemm_bf16_ln_bwd_pf", ctypes.byref(d), A.data_ptr(), Bw.data_ptr(), scratch.data_ptr(), x.data_ptr(), w.data_ptr(),
             mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), _p(dx_bf16), _p(dres), _p(dw), _p(db),
             lnws.data_ptr(), lnws.numel() * 4, ws.data_ptr(), ws.numel() * 4, _stream(), pf)
        return dx
    return _ln_param_grads(w, b, M, N, x.device, kernel)


def attention_fwd(qkv, B, L, heads, dh, prec, out_bf16=None):
    out = torch.empty(B * L, heads * dh, dtype=torch.float32, device=qkv.device)
    lse = torch.empty(B, heads, L, dtype=torch.float32, device=qkv.device)
    call("unetr_attention_fwd", qkv.data_ptr(), out.data_ptr(), _p(out_bf16), lse.data_ptr(), B, L, heads, dh, float(dh) ** -0.5, prec, _stream())
    return out, lse


def attention_bwd(qkv, out, dout, lse, B, L, heads, dh, prec, dqkv_bf16=None):
    dqkv = torch.empty_like(qkv)
    delta = torch.empty_like(lse)
    call("unetr_attention_bwd", qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), _p(dqkv_bf16),
         delta.data_ptr(),
         B, L, heads, dh, float(dh) ** -0.5, prec, _stream())
    return dqkv


def attention_bf16_fwd(qkvb, B, L, heads, dh, out_bf16, out=None, pf=None):
    lse = torch.empty(B, heads, L, dtype=torch.float32, device=qkvb.device)
    call("unetr_attention_bf16_fwd_pf", qkvb.data_ptr(), _p(out), out_bf16.data_ptr(), lse.data_ptr(), B, L, heads, dh, float(dh) ** -0.5, _stream(), pf)
    return lse


def attention_bf16_bwd(qkvb, outb, doutb, lse, B, L, heads, dh, dqkv=None, pf=None):
    dqkvb = torch.empty_like(qkvb)
    delta = torch.empty_like(lse)
    call("unetr_attention_bf16_bwd_pf", qkvb.data_ptr(), outb.data_ptr(), doutb.data_ptr(), lse.data_ptr(), _p(dqkv), dqkvb.data_ptr(),
         delta.data_ptr(), B, L, heads, dh, float(dh) ** -0.5, _stream(), pf)
    return dqkvb


def conv3(x, ldx, w, dims, prec, mode=0, out=None, ldo=None, accumulate=False):
    """3x3x3 conv (mode 0: w[Cout,Cin,3,3,3] applied to x with Cin channels) or its data gradient
    (mode 1: x carries Cout channels, result has Cin channels)."""
    B, D, H, W = dims
    cout_w, cin_w = w.shape[0], w.shape[1]
    cin, cout = (cin_w, cout_w) if mode == 0 else (cout_w, cin_w)
    if cout % 16 != 0:
        return conv_fwd(x, ldx, conv_pack(w, mode), dims, cin, cout, 3, prec, out=out, ldo=ldo, accumulate=accumulate)
    wp = conv_pack_get(w, mode, prec)
    if out is None:
        out = torch.empty(B, D, H, W, cout, dtype=act_dtype(prec), device=x.device)
        ldo = cout
    call("unetr_conv3_fwd", x.data_ptr(), ldx, wp.data_ptr(), out.data_ptr(), ldo, int(accumulate), B, D, H, W, cin, cout, prec, _stream())
    return out


def conv3_fused(x, ldx, w, w3, dims, prec):
    """First half of a residual block in one launch: c = conv3x3x3(x, w) with its InstanceNorm statistics and, when w3 is
    given, c3 = conv1x1x1(x, w3) with its statistics (both convs read the same staged window).  Returns
    (c, stats, c3, stats3) or None when the shape has to take the unfused kernels."""
    B, D, H, W = dims
    cout, cin = w.shape[0], w.shape[1]
    if cout % 16 != 0:
        return None
    wp, c, st, wp3, c3, st3, x_f32 = _conv3_front(x, w, w3, dims, prec, (cout, 2))
    ws = workspace(x.device)
    rc = call_rc("unetr_conv3_fwd_fused", x.data_ptr(), ldx, wp.data_ptr(), c.data_ptr(), cout, st.data_ptr(), _p(wp3), _p(c3), cout,
                 _p(st3), IN_EPS, B, D, H, W, cin, cout, prec, x_f32, ws.data_ptr(), ws.numel() * 4, _stream())
    return (c, st, c3, st3) if rc == 0 else None


def _conv3_front(x, w, w3, dims, prec, stat_shape, store3=True):
    """what conv3_fused and conv3_parts set up alike: (packed w, c, its statistics buffer [B, *stat_shape], the same three for the
    1x1x1 conv w3 or None each, x_f32).  store3=False: the 1x1x1 output is not allocated."""
    B, D, H, W = dims

    def conv(wk, kind, store):
        return (conv_pack_get(wk, kind, prec), torch.empty(B, D, H, W, w.shape[0], dtype=act_dtype(prec), device=x.device) if store else None,
                torch.empty(B, *stat_shape, dtype=torch.float32, device=x.device))
    x_f32 = int(prec == _capi.PREC_BF16 and x.dtype == torch.float32)      # the image in front of encoder1
    return conv(w, 0, True) + (conv(w3, 2, store3) if w3 is not None else (None, None, None)) + (x_f32,)


CONV3_MAX_ROWS = 1024        # = UNETR_CONV3_MAX_ROWS (include/unetr_hip.h)


def in_fuse_level():
    """UNETR_AMD_IN_FUSE (tuning / A-B hook), a bit mask: 1 = the forward statistics finalize rides in the prologue of the apply
    kernel (no finalize launches in the forward of a residual block), 2 = the backward statistics of a block's first norm are
    formed in the epilogue of the data-gradient conv that produces its gradient (no reduction pass, no finalize launch)."""
    return int(os.environ.get("UNETR_AMD_IN_FUSE", "3"))


def conv3_parts(x, ldx, w, w3, dims, prec, store3=True):
    """conv3_fused without the statistics finalize: returns (c, part, c3, part3, rows) -- part* = InstanceNorm partial rows
    [B, rows, 2, Cout] that instnorm_apply_fin reduces in its prologue -- or None when the shape takes another route.
    store3=False: the 1x1x1 branch is not stored (c3 is None), only its statistics rows are formed."""
    B, D, H, W = dims
    cout, cin = w.shape[0], w.shape[1]
    if cout % 16 != 0 or cout > 128:
        return None
    wp, c, part, wp3, c3, part3, x_f32 = _conv3_front(x, w, w3, dims, prec, (CONV3_MAX_ROWS, 2, cout), store3)
    rows = ctypes.c_int(0)
    rc = call_rc("unetr_conv3_fwd_parts", x.data_ptr(), ldx, wp.data_ptr(), c.data_ptr(), cout, part.data_ptr(), _p(wp3), _p(c3), cout,
                 _p(part3), ctypes.byref(rows), B, D, H, W, cin, cout, prec, x_f32, _stream())
    return (c, part, c3, part3, rows.value) if rc == 0 else None


def instnorm_apply_fin(x, part, rows, B, V, C, lrelu, x2=None, part_b=None, rows_b=0, out=None, ldo=None):
    """instnorm_apply with the statistics formed in the kernel's prologue from partial rows; returns (y, stats, stats_b) or None"""
    y, ldy, sa, sb = _apply_fin_outputs(x, B, C, out, ldo, x2 is not None)
    rc = call_rc("unetr_instnorm_apply_fin", x.data_ptr(), C, part.data_ptr(), rows, _p(x2), C, _p(part_b), rows_b, sa.data_ptr(), _p(sb),
                 IN_EPS, y.data_ptr(), ldy, B, V, C, int(lrelu), _a16(x), _stream())
    return (y, sa, sb) if rc == 0 else None


def _apply_fin_outputs(x, B, C, out, ldo, dual):
    """(y, its row pitch, statistics of x, statistics of the second branch or None) of the two instnorm_apply_fin forms"""
    y = torch.empty_like(x) if out is None else out
    sa = torch.empty(B, C, 2, dtype=torch.float32, device=x.device)
    return y, (C if out is None else ldo), sa, (torch.empty(B, C, 2, dtype=torch.float32, device=x.device) if dual else None)


IN_IMG_MAX_ROWS = 512       # = UNETR_IN_IMG_MAX_ROWS


def instnorm_apply_fin_img(x, part, rows, img, cin, w3, part_b, rows_b, B, V, C, out=None, ldo=None):
    """block end of the residual block on the image: lrelu(norm(x) + norm(conv1x1x1(img; w3))) with the 1x1x1 branch formed from the
    image in the kernel; returns (y, stats, stats_b) or None"""
    y, ldy, sa, sb = _apply_fin_outputs(x, B, C, out, ldo, True)
    rc = call_rc("unetr_instnorm_apply_fin_img", x.data_ptr(), C, part.data_ptr(), rows, img.data_ptr(), cin, w3.data_ptr(), part_b.data_ptr(), rows_b,
                 sa.data_ptr(), sb.data_ptr(), IN_EPS, y.data_ptr(), ldy, B, V, C, 1, _a16(x), _stream())
    return (y, sa, sb) if rc == 0 else None


def instnorm_bwd_img(dy, lddy, x, sa, img, cin, w3, sb, B, V, C):
    """backward of the same block end: (dx of the 3x3x3 branch, dw3 partial rows [rows, C * cin], rows) or None"""
    if dy.dtype != x.dtype:
        dy = dy.to(x.dtype).contiguous(); lddy = dy.stride(-2)
    dx = torch.empty_like(x)
    part = torch.empty(IN_IMG_MAX_ROWS, C * cin, dtype=torch.float32, device=x.device)
    rows = ctypes.c_int(0)
    ws = workspace(x.device)
    rc = call_rc("unetr_instnorm_bwd_img", dy.data_ptr(), lddy, x.data_ptr(), C, sa.data_ptr(), img.data_ptr(), cin, w3.data_ptr(), sb.data_ptr(),
                 dx.data_ptr(), C, part.data_ptr(), ctypes.byref(rows), B, V, C, 1, ws.data_ptr(), ws.numel() * 4, _a16(x), _stream())
    return (dx, part, rows.value) if rc == 0 else None


def conv3_dgrad_stats(dy, w, xn, stats, dims, prec):
    """da = conv3x3x3^T(dy; w) together with the partial sums of the InstanceNorm backward of xn's norm (the norm whose
    lrelu'd output the conv read): returns (da, part, rows) or None when the shape takes the unfused route"""
    B, D, H, W = dims
    cout, cin = w.shape[0], w.shape[1]
    if cin % 16 != 0 or cin > 128 or xn.stride(-2) != cin:
        return None
    wp = conv_pack_get(w, 1, prec)
    da = torch.empty(B, D, H, W, cin, dtype=act_dtype(prec), device=dy.device)
    part = torch.empty(B, CONV3_MAX_ROWS, 2, cin, dtype=torch.float32, device=dy.device)
    rows = ctypes.c_int(0)
    rc = call_rc("unetr_conv3_dgrad_stats", dy.data_ptr(), cout, wp.data_ptr(), da.data_ptr(), cin, xn.data_ptr(), cin, stats.data_ptr(),
                 part.data_ptr(), ctypes.byref(rows), B, D, H, W, cin, cout, prec, _stream())
    if rc != 0:
        return None
    return da, part, rows.value


def instnorm_bwd_apply_fin(dy, lddy, x, sa, part, rows, nsp, B, V, C, lrelu):
    """dx of y = lrelu?(norm(x)) from dy and the partial sums `part` [B, rows, nsp, C]; None when unsupported"""
    r = _bwd_apply_fin(dy, lddy, x, sa, None, None, part, rows, nsp, B, V, C, lrelu)
    return r[0] if r is not None else None


def _bwd_apply_fin(dy, lddy, x, sa, x2, sb, part, rows, nsp, B, V, C, lrelu):
    """the one call behind instnorm_bwd_apply_fin and its dual form (x2, sb: the second normalised branch): (dx, dx2 or None) or None"""
    dx = torch.empty_like(x)
    dx2 = torch.empty_like(x2) if x2 is not None else None
    ld2 = C if x2 is not None else 0
    rc = call_rc("unetr_instnorm_bwd_apply_fin", dy.data_ptr(), lddy, x.data_ptr(), C, sa.data_ptr(), _p(x2), ld2, _p(sb), part.data_ptr(), rows, nsp,
                 dx.data_ptr(), C, _p(dx2), ld2, B, V, C, int(lrelu), _a16(x), _stream())
    return (dx, dx2) if rc == 0 else None


def out_fuse_enabled():
    """UNETR_AMD_OUT_FUSE=0 (A/B hook): decoder2's block end is stored and the out conv reads it, as every other block end"""
    return os.environ.get("UNETR_AMD_OUT_FUSE", "1") != "0"


def outconv_in_fwd(c2, p2, rows2, c3, p3, rows3, wo, bo, B, V, C):
    """logits of the out conv on lrelu(norm(c2) + norm(c3)) without storing that tensor (csrc/norm_misc.hip: outconv_in_fwd_kernel);
    returns (logits [B, Cout, V] fp32, stats of c2, stats of c3) or None when the shape takes the unfused sequence"""
    cout = wo.shape[0]
    if wo.shape[1] != C or not wo.is_contiguous():
        return None
    logits = torch.empty(B, cout, V, dtype=torch.float32, device=c2.device)
    sa = torch.empty(B, C, 2, dtype=torch.float32, device=c2.device)
    sb = torch.empty(B, C, 2, dtype=torch.float32, device=c2.device)
    rc = call_rc("unetr_outconv_in_fwd", c2.data_ptr(), C, p2.data_ptr(), rows2, c3.data_ptr(), C, p3.data_ptr(), rows3, sa.data_ptr(), sb.data_ptr(),
                 IN_EPS, wo.data_ptr(), _p(bo), logits.data_ptr(), B, V, C, cout, _a16(c2), _stream())
    return (logits, sa, sb) if rc == 0 else None


def outconv_in_bwd(dl, c2, s2, c3, s3, wo, bo, B, V, C):
    """backward of outconv_in_fwd up to the block end's normalisation: (dout in the storage type of c2, InstanceNorm backward partial
    rows [B, rows, 3, C], rows, dwo, dbo)"""
    cout = wo.shape[0]
    rows = _capi.load().unetr_outconv_in_bwd_rows(B, V, C, _a16(c2))
    if rows <= 0:
        raise RuntimeError("unetr_outconv_in_bwd: shape accepted by the forward kernel is declined by backward")
    dl = dl.contiguous()
    dout = torch.empty_like(c2)
    part = torch.empty(B, rows, 3, C, dtype=torch.float32, device=c2.device)
    gw, gb = _gout(wo), _gout(bo)
    dw = gw if gw is not None else torch.empty_like(wo)
    db = gb if gb is not None else torch.empty(cout, dtype=torch.float32, device=c2.device)
    ws = workspace(c2.device)
    call("unetr_outconv_in_bwd", dl.data_ptr(), c2.data_ptr(), C, s2.data_ptr(), c3.data_ptr(), C, s3.data_ptr(), wo.data_ptr(), dout.data_ptr(), C,
         part.data_ptr(), dw.data_ptr(), db.data_ptr(), B, V, C, cout, ws.data_ptr(), ws.numel() * 4, _a16(c2), _stream())
    return dout, part, rows, dw, db


def instnorm_bwd_apply_fin_dual(dy, lddy, x, sa, x2, sb, part, rows, B, V, C):
    """(dx, dx2) of y = lrelu(norm(x) + norm(x2)) from dy and the partial sums `part` [B, rows, 3, C]; None when unsupported"""
    return _bwd_apply_fin(dy, lddy, x, sa, x2, sb, part, rows, 3, B, V, C, True)


def conv3_dgrad_fused(dc1, dc3, w1, w3, dx, dims, prec):
    """dx = conv3x3x3^T(dc1; w1) + conv1x1x1^T(dc3; w3) in one launch (the input gradient of a residual block);
    returns False when the shape has to take the two-kernel route."""
    B, D, H, W = dims
    cout, cin = w1.shape[0], w1.shape[1]
    if cin % 16 != 0:
        return False
    wp = conv_pack_get(w1, 1, prec)
    w3t = conv_pack_get(w3, 3, prec)
    ws = workspace(dc1.device)
    rc = call_rc("unetr_conv3_dgrad_fused", dc1.data_ptr(), cout, wp.data_ptr(), dc3.data_ptr(), cout, w3.data_ptr(), w3t.data_ptr(), dx.data_ptr(), cin,
                 B, D, H, W, cin, cout, prec, ws.data_ptr(), ws.numel() * 4, _stream())
    return rc == 0


def conv3_wgrad(x, ldx, dy, lddy, dims, cin, cout, prec, out=None, dy3=None, out3=None):
    """dw of the 3x3x3 conv; with dy3/out3 also the weight gradient of the 1x1x1 conv sharing the input x"""
    return _conv3_wgrad_queued(None, x, ldx, dy, lddy, dims, cin, cout, prec, out, dy3, out3)[0]


def _conv3_wgrad_queued(st, x, ldx, dy, lddy, dims, cin, cout, prec, out=None, dy3=None, out3=None):
    """conv3_wgrad for a block's backward: (dw, queued).  st = the ArenaState owning `out` (and `out3`), or None.  With a state the
    kernel leaves its per-workgroup partial sums in a buffer of its own and the reduction joins the ONE grouped reduce launch at
    the end of the backward pass (queued = True) -- where the shape allows; otherwise dw is complete on return (queued = False)."""
    B, D, H, W = dims
    dw = out if out is not None else torch.empty(cout, cin, 3, 3, 3, dtype=torch.float32, device=x.device)
    x_f32 = int(prec == _capi.PREC_BF16 and x.dtype == torch.float32)
    if st is not None:
        rows = _capi.load().unetr_conv3_wgrad_rows(B, D, H, W, cin, cout, prec, x_f32, int(dy3 is not None))
        n, n3 = 27 * cin * cout, (cin * cout if dy3 is not None else 0)
        if rows > 0 and rows * (n + n3) * 4 <= (256 << 20):
            part = torch.empty(rows * (n + n3), dtype=torch.float32, device=x.device)
            got = ctypes.c_long(0)
            rc = call_rc("unetr_conv3_wgrad_parts", x.data_ptr(), ldx, dy.data_ptr(), lddy, _p(dy3), cout, part.data_ptr(), part.numel() * 4,
                         ctypes.byref(got), B, D, H, W, cin, cout, prec, x_f32, _stream())
            if rc == 0:
                g = got.value
                st.queue_reduce(part, dw, n, g)
                if dy3 is not None:
                    st.queue_reduce(part[g * n:], out3, n3, g)
                return dw, True
    ws = workspace(x.device)
    call("unetr_conv3_wgrad", x.data_ptr(), ldx, dy.data_ptr(), lddy, dw.data_ptr(), _p(dy3), cout, _p(out3),
         B, D, H, W, cin, cout, prec, x_f32, ws.data_ptr(), ws.numel() * 4, _stream())
    return dw, False


def conv_pack(w, mode):
    """torch Conv3d weight [Cout,Cin,k,k,k] -> GEMM operand layout (mode 0 fwd, mode 1 dgrad)."""
    cout, cin, ks = w.shape[0], w.shape[1], w.shape[2]
    wp = torch.empty(w.numel(), dtype=torch.float32, device=w.device)
    call("unetr_conv_pack_weight", w.data_ptr(), wp.data_ptr(), cin, cout, ks, mode, _stream())
    return wp


def conv_fwd(x, ldx, wpack, dims, cin, cout, ks, prec, out=None, ldo=None, accumulate=False):
    """x: rows [B*D*H*W, cin] pitch ldx -> y rows [.., cout]"""
    B, D, H, W = dims
    boundary = prec == _capi.PREC_BF16       # generic im2col-loader GEMM family, fp32 storage only (shapes the dedicated kernels decline)
    y, ldy = out, ldo
    if boundary:
        x, ldx = _f32_rows(x, ldx, cin)
    if boundary or out is None:
        y, ldy = torch.empty(B, D, H, W, cout, dtype=torch.float32, device=x.device), cout
        if accumulate and out is not None:
            y.copy_(out)
    ws = workspace(x.device)
    call("unetr_conv_gemm_fwd", x.data_ptr(), ldx, wpack.data_ptr(), y.data_ptr(), ldy, int(accumulate), B, D, H, W, cin, cout, ks,
         prec, ws.data_ptr(), ws.numel() * 4, _stream())
    return _act_rows(y, prec, out) if boundary else y


def conv_wgrad(x, ldx, dy, lddy, dims, cin, cout, ks, prec, out=None):
    B, D, H, W = dims
    dw = out if out is not None else torch.empty(cout, cin, ks, ks, ks, dtype=torch.float32, device=x.device)
    ws = workspace(x.device)
    x, ldx = _f32_rows(x, ldx, cin)
    dy, lddy = _f32_rows(dy, lddy, cout)
    call("unetr_conv_gemm_wgrad", x.data_ptr(), ldx, dy.data_ptr(), lddy, dw.data_ptr(), B, D, H, W, cin, cout, ks, prec,
         ws.data_ptr(), ws.numel() * 4, _stream())
    return dw


def instnorm_stats(x, ld, B, V, C):
    stats = torch.empty(B, C, 2, dtype=torch.float32, device=x.device)
    ws = workspace(x.device)
    call("unetr_instnorm_stats", x.data_ptr(), ld, B, V, C, IN_EPS, stats.data_ptr(), ws.data_ptr(), ws.numel() * 4, _a16(x), _stream())
    return stats


def instnorm_apply(x, sa, B, V, C, lrelu, x2=None, sb=None, out=None, ldo=None):
    """``out`` / ``ldo``: write into an existing buffer with row pitch ldo (the skip half of a concatenation buffer)"""
    y = torch.empty_like(x) if out is None else out
    call("unetr_instnorm_apply", x.data_ptr(), C, sa.data_ptr(), x2.data_ptr() if x2 is not None else None, C,
         sb.data_ptr() if sb is not None else None, y.data_ptr(), C if out is None else ldo, B, V, C, int(lrelu), _a16(x), _stream())
    return y


def instnorm_bwd(dy, lddy, x, sa, B, V, C, lrelu, x2=None, sb=None):
    if dy.dtype != x.dtype:
        dy = dy.to(x.dtype).contiguous(); lddy = dy.stride(-2)
    dx = torch.empty_like(x)
    dx2 = torch.empty_like(x2) if x2 is not None else None
    ws = workspace(x.device)
    call("unetr_instnorm_bwd", dy.data_ptr(), lddy, x.data_ptr(), C, sa.data_ptr(), x2.data_ptr() if x2 is not None else None, C,
         sb.data_ptr() if sb is not None else None, dx.data_ptr(), C, dx2.data_ptr() if dx2 is not None else None, C,
         B, V, C, int(lrelu), ws.data_ptr(), ws.numel() * 4, _a16(x), _stream())
    return dx, dx2


def _tconv_as_gemm(prec, M, cin, cout, ld_in):
    """the small transposed convs (768 channels at 6^3, 64 / 128 at 12^3) go through the bf16-storage GEMM: few voxels, many
    channels -- exactly where the dedicated voxel-tile kernels decline and the gather-loader GEMM family was 3-6x slower"""
    return (prec == _capi.PREC_BF16 and cin % 64 == 0 and M % 8 == 0 and ld_in == cin and M < 8192)


def tconv_fwd(x, ldx, w, dims, cin, cout, prec, out=None, ldo=None):
    B, D, H, W = dims
    adt = act_dtype(prec)
    if out is None:
        out = torch.empty(B, 2 * D, 2 * H, 2 * W, cout, dtype=adt, device=x.device)
        ldo = cout
    M = B * D * H * W
    if _tconv_as_gemm(prec, M, cin, cout, ldx):
        xb = _twin(x).view(M, cin)             # (a bf16 feature map is its own operand; tokens bring their bf16 twin)
        if out.dtype == torch.bfloat16 and cout % 4 == 0 and ldo % 4 == 0:
            # tap-major weight pack [Cin][tap][Cout] (re-packed with the conv weights after every update): the GEMM's epilogue
            # writes each (voxel, tap) row of Cout channels straight to its output voxel -- no fp32 [M, 8 Cout] intermediate, no
            # pixel-shuffle launch
            wp = conv_pack_get(w, 4, prec).view(torch.bfloat16)
            gemm_bf16(xb, wp, M, 8 * cout, cin, b_kn=True, Cb=out, ldcb=ldo, tc=(D, H, W, cout))
            return out, xb
        tmp = torch.empty(M, 8 * cout, dtype=torch.float32, device=x.device)
        gemm_bf16(xb, weight_bf16(w).view(cin, 8 * cout), M, 8 * cout, cin, b_kn=True, C=tmp)
        call("unetr_pixel_shuffle2", tmp.data_ptr(), out.data_ptr(), ldo, B, D, H, W, cout, _a16(out), _stream())
        return out, xb
    if prec == _capi.PREC_BF16 and x.dtype != adt:
        x = x.to(adt).contiguous(); ldx = cin      # (fp32 tokens in front of a shape the GEMM form does not take)
    tail = _tconv_tail(dims, cin, cout, prec, x.device)

    def boundary():
        x32, l32 = _f32_rows(x, ldx, cin)
        o32 = torch.empty(B, 2 * D, 2 * H, 2 * W, cout, dtype=torch.float32, device=x.device)
        call("unetr_tconv_fwd", x32.data_ptr(), l32, w.data_ptr(), o32.data_ptr(), cout, *tail)
        # (through the row-copy kernel, not Tensor.copy_: `out` may be a view handed out by TconvFn.forward -- the skip half of
        # a concatenation buffer -- and a torch in-place op on it inside a custom Function invalidates the view's grad_fn)
        o16 = _act_rows(o32, prec)
        call("unetr_copy_rows", out.data_ptr(), ldo, o16.data_ptr(), cout, B * 8 * D * H * W, cout, 0, _a16(out), _stream())
    _tconv_ladder("fwd", (x.data_ptr(), ldx, w.data_ptr(), out.data_ptr(), ldo) + tail, prec, boundary)
    return out, None


def _tconv_tail(dims, cin, cout, prec, device):
    """the arguments every transposed-conv kernel ends with"""
    ws = workspace(device)
    return (*dims, cin, cout, prec, ws.data_ptr(), ws.numel() * 4, _stream())


def _tconv_ladder(which, args, prec, boundary):
    """The ladder of tconv_fwd / tconv_dgrad / tconv_wgrad: the dedicated kernel unetr_tconv2_<which>; where it declines the shape,
    the generic GEMM family's unetr_tconv_<which> -- on the same arguments in the fp32-storage modes, through `boundary()` (which
    casts to fp32 and back) in bf16 mode."""
    if call_rc("unetr_tconv2_" + which, *args) == 0:
        return
    if prec == _capi.PREC_BF16:
        boundary()
    else:
        call("unetr_tconv_" + which, *args)


def tconv_bwd(x, ldx, xb, dy, lddy, w, dims, cin, cout, prec, need_dx):
    """(dx or None, dw as autograd wants it) of the transposed conv; xb: the bf16 input the GEMM form of forward kept"""
    B, D, H, W = dims
    M = B * D * H * W
    if xb is not None:
        dyg = torch.empty(M, 8 * cout, dtype=torch.bfloat16, device=dy.device)
        call("unetr_pixel_unshuffle2_bf16", dy.data_ptr(), lddy, dyg.data_ptr(), B, D, H, W, cout, _a16(dy), _stream())
        dx = None
        if need_dx:
            dx = torch.empty(B, D, H, W, cin, dtype=x.dtype, device=dy.device)        # fp32 for tokens, bf16 for feature maps
            wb = weight_bf16(w).view(cin, 8 * cout)
            if dx.dtype == torch.bfloat16:
                gemm_bf16(dyg, wb, M, cin, 8 * cout, Cb=dx.view(M, cin))
            else:
                gemm_bf16(dyg, wb, M, cin, 8 * cout, C=dx.view(M, cin))
        # dw[Cin, Cout*8] = x^T dyg is torch's [Cin, Cout, 2, 2, 2] as it stands: joins the grouped end-of-backward launch
        dw = wgrad_or_defer(None, None, prec, w, xb, dyg)
        if dw is not None:
            dw = dw.view_as(w)
        return dx, dw
    if prec == _capi.PREC_BF16 and x.dtype != torch.bfloat16:
        x = x.to(torch.bfloat16).contiguous(); ldx = cin
    if prec == _capi.PREC_BF16 and dy.dtype != torch.bfloat16:
        dy = dy.to(torch.bfloat16).contiguous(); lddy = cout
    dx = tconv_dgrad(dy, lddy, w, dims, cin, cout, prec) if need_dx else None
    st, gw = grad_arena.dest(w)
    if st is not None:
        # arena mode: the partial sums of the weight gradient stay in a buffer of their own; their reduction joins the grouped launch
        # at the end of the backward pass
        rows = _capi.load().unetr_tconv2_wgrad_rows(B, D, H, W, cin, cout)
        n = cin * cout * 8
        if rows > 0:
            part = torch.empty(rows * n, dtype=torch.float32, device=x.device)
            got = ctypes.c_long(0)
            if call_rc("unetr_tconv2_wgrad_parts", x.data_ptr(), ldx, dy.data_ptr(), lddy, part.data_ptr(), part.numel() * 4, ctypes.byref(got),
                       B, D, H, W, cin, cout, prec, _stream()) == 0:
                st.queue_reduce(part, gw, n, got.value)
                return dx, _ret(w, gw, deferred=True)
    dw = tconv_wgrad(x, ldx, dy, lddy, dims, cin, cout, prec, out=gw)
    return dx, _ret(w, dw)


def tconv_dgrad(dy, lddy, w, dims, cin, cout, prec):
    B, D, H, W = dims
    dx = torch.empty(B, D, H, W, cin, dtype=act_dtype(prec), device=dy.device)
    tail = _tconv_tail(dims, cin, cout, prec, dy.device)

    def boundary():
        d32, l32 = _f32_rows(dy, lddy, cout)
        x32 = torch.empty(B, D, H, W, cin, dtype=torch.float32, device=dy.device)
        call("unetr_tconv_dgrad", d32.data_ptr(), l32, w.data_ptr(), x32.data_ptr(), cin, 0, *tail)
        _act_rows(x32, prec, out=dx)
    _tconv_ladder("dgrad", (dy.data_ptr(), lddy, w.data_ptr(), dx.data_ptr(), cin, 0) + tail, prec, boundary)
    return dx


def tconv_wgrad(x, ldx, dy, lddy, dims, cin, cout, prec, out=None):
    dw = out if out is not None else torch.empty(cin, cout, 2, 2, 2, dtype=torch.float32, device=x.device)
    tail = _tconv_tail(dims, cin, cout, prec, x.device)

    def boundary():
        x32, lx = _f32_rows(x, ldx, cin)
        d32, ld = _f32_rows(dy, lddy, cout)
        call("unetr_tconv_wgrad", x32.data_ptr(), lx, d32.data_ptr(), ld, dw.data_ptr(), *tail)
    _tconv_ladder("wgrad", (x.data_ptr(), ldx, dy.data_ptr(), lddy, dw.data_ptr()) + tail, prec, boundary)
    return dw


# --------------------------------------------------------------------------------- ViT encoder functions
class PatchEmbedFn(torch.autograd.Function):
    """MONAI PatchEmbeddingBlock(pos_embed="perceptron"): rearrange + Linear + position embedding."""

    @staticmethod
    def forward(ctx, x_in, w, b, pos, patch, prec):
        _require_gpu(x_in)
        x_in = x_in.contiguous()
        B, C, D, H, W = x_in.shape
        L = (D // patch) * (H // patch) * (W // patch)
        pd = C * patch ** 3
        hid = w.shape[0]
        patches = ctx.pb = None
        if _bf16_path(prec, pd) and (B * L) % 8 == 0 and hid % 8 == 0:
            # the bf16 GEMM operand straight from the gather kernel (no fp32 patch matrix, no cast pass).  Only where backward's
            # weight gradient can take the bf16 grouped launch (wgrad_or_defer: rows and both widths multiples of 8): its fp32
            # fallback needs the fp32 patch matrix this branch does not keep (e.g. 48^3 at batch 1: 27 token rows)
            z = torch.empty(B * L, hid, dtype=torch.float32, device=x_in.device)
            ctx.pb = torch.empty(B * L, pd, dtype=torch.bfloat16, device=x_in.device)
            call("unetr_patch_gather", x_in.data_ptr(), None, ctx.pb.data_ptr(), B, C, D, H, W, patch, _stream())
            gemm_bf16(ctx.pb, weight_bf16(w), B * L, hid, pd, C=z, bias=b, res=pos, ldr=hid, res_mod=L)
        else:
            patches = torch.empty(B * L, pd, dtype=torch.float32, device=x_in.device)
            call("unetr_patch_gather", x_in.data_ptr(), patches.data_ptr(), None, B, C, D, H, W, patch, _stream())
            z = linear_fwd(patches, w, b, prec, res=pos, res_mod=L)
        ctx.save_for_backward(patches, w, b, pos)
        ctx.meta = (B, L, hid, prec)
        return z

    @staticmethod
    def backward(ctx, dz):
        patches, w, b, pos = ctx.saved_tensors
        B, L, hid, prec = ctx.meta
        dz = dz.contiguous()
        dw = wgrad_or_defer(dz, patches, prec, w, _twin(dz) if ctx.pb is not None else None, ctx.pb)
        db = colsum_or_defer(dz, B * L, hid, hid, b)
        dpos = colsum_or_defer(dz, B, L * hid, L * hid, pos, view_shape=(1, L, hid))
        return None, dw, db, dpos, None, None


# The route of one transformer block, decided once in forward from (prec, M, hid, mlp, dh) and the switches; backward and the
# checkpoint recompute read it.  fast: bf16-stored operands for every GEMM (fp32 copies stay only where a kernel reads them);
# b16att: q/k/v stay bf16 from the GEMM epilogue to the attention kernels' LDS-DMA; x3ride / x3ride_qkv (bf16x3): the LayerNorm
# rides on the GEMM with K = mlp (forward of the next norm1, backward of norm2) / K = 3 hid (backward of norm1).
BlockRoute = collections.namedtuple("BlockRoute", "fast b16att x3ride x3ride_qkv")
# What backward needs of a block's forward, None where the route has no such tensor: the fp32 activations and LayerNorm statistics
# (y1 y2 a: fp32 routes only; att: not with b16att; u, the pre-activation that only GELU' reads: training only), then the bf16
# operands of the weight-gradient GEMMs (fast route only).
BlockActs = collections.namedtuple("BlockActs", "y1 m1 r1 qkv att lse x1 y2 m2 r2 u a y1b attb y2b ab")


def _block_route(prec, M, hid, mlp, dh):
    fast = _bf16_path(prec, hid, mlp) and M % 8 == 0          # (the bf16 weight-gradient kernel wants whole 8-token groups)
    x3 = prec == _capi.PREC_BF16X3 and ln_ride_enabled()
    return BlockRoute(fast, fast and dh == 64, x3 and x3_ride_ok(M, hid, mlp), x3 and x3_ride_ok(M, hid, 3 * hid))


def _tblock_forward(x, n1w, n1b, wqkv, wp, bp, n2w, n2b, w1, b1, w2, b2, B, L, heads, prec, route, train, next_ln=None, emit_twin=False,
                    next_wqkv=None):
    """kernels of one transformer block; returns (x2, BlockActs).  next_ln = (gamma, beta) of the LayerNorm the next layer starts
    with: computed by the kernel that forms x2 and left on x2 (_stash_ln).  next_wqkv: the qkv weight of that next layer,
    prefetched by the same kernel.  bf16 path: every non-GEMM launch prefetches the weights of the GEMM(s) behind it (_prefetch)"""
    M, hid = x.shape
    dh, mlp = hid // heads, w1.shape[0]
    f32 = dict(dtype=torch.float32, device=x.device)
    if route.fast:
        qkv = torch.empty(M, 3 * hid, dtype=torch.bfloat16 if route.b16att else torch.float32, device=x.device)
        pre = _stashed_ln(x, n1w, n1b)       # norm1(x) may have been formed by the kernel that produced x
        if pre is not None:
            y1b, m1, r1 = pre
        else:
            y1b = bf16_like(x)
            _, m1, r1 = layernorm_fwd(x, n1w, n1b, bf16_out=y1b, want_fp32=False, pf=_prefetch("ln1_fwd", wqkv))
        gemm_bf16(y1b, weight_bf16(wqkv), M, 3 * hid, hid, C=None if route.b16att else qkv, Cb=qkv if route.b16att else None)
        attb, att = bf16_like(x), None
        if route.b16att:
            lse = attention_bf16_fwd(qkv, B, L, heads, dh, attb, pf=_prefetch("attn_fwd", wp, w1))
        else:
            att, lse = attention_fwd(qkv, B, L, heads, dh, prec, out_bf16=attb)
        x1 = torch.empty(M, hid, **f32)
        gemm_bf16(attb, weight_bf16(wp), M, hid, hid, C=x1, bias=bp, res=x, ldr=hid)
        u = torch.empty(M, mlp, **f32) if train else None
        ab = torch.empty(M, mlp, dtype=torch.bfloat16, device=x.device)
        y2b = bf16_like(x)
        _, m2, r2 = layernorm_fwd(x1, n2w, n2b, bf16_out=y2b, want_fp32=False, pf=_prefetch("ln2_fwd", w2))
        gemm_bf16(y2b, weight_bf16(w1), M, mlp, hid, Cb=ab, bias=b1, act=1, pre=u)
        x2 = torch.empty(M, hid, **f32)
        if next_ln is not None and not emit_twin:      # (a tapped block writes the bf16 twin of x2 from its own epilogue)
            xn = bf16_like(x)
            mn, rn = gemm_bf16_ln_fwd(ab, weight_bf16(w2), M, hid, mlp, x2, next_ln[0], next_ln[1], xn, bias=b2, res=x1, ldr=hid,
                                      pf=_prefetch("ln1_fwd", next_wqkv))
            _stash_ln(x2, next_ln[0], next_ln[1], xn, mn, rn)
        else:
            # emit_twin: this block's output also feeds a skip-path transposed conv that reads bf16 tokens (its GEMM form):
            # the epilogue writes the bf16 copy next to the fp32 residual stream (was a separate cast launch)
            x2b = bf16_like(x) if emit_twin else None
            gemm_bf16(ab, weight_bf16(w2), M, hid, mlp, C=x2, Cb=x2b, bias=b2, res=x1, ldr=hid)
            if x2b is not None:
                _attach_twin(x2, x2b)
        return x2, BlockActs(None, m1, r1, qkv, att, lse, x1, None, m2, r2, u, None, y1b, attb, y2b, ab)
    pre = _stashed_ln(x, n1w, n1b) if route.x3ride else None      # (bf16x3: norm1(x) may have ridden on the GEMM that produced x)
    y1, m1, r1 = pre if pre is not None else layernorm_fwd(x, n1w, n1b)
    qkv = linear_fwd(y1, wqkv, None, prec)
    att, lse = attention_fwd(qkv, B, L, heads, dh, prec)
    x1 = linear_fwd(att, wp, bp, prec, res=x)
    y2, m2, r2 = layernorm_fwd(x1, n2w, n2b)
    u = torch.empty(M, mlp, **f32)
    a = linear_fwd(y2, w1, b1, prec, act=1, pre=u)
    if route.x3ride and next_ln is not None:
        # the next block's norm1 rides on the split-K sum of linear2 (as in bf16 mode): no reduce launch, no LayerNorm launch
        x2 = torch.empty(M, hid, **f32)
        xn = torch.empty_like(x2)
        mn, rn = gemm_bf16_ln_fwd(a, w2, M, hid, mlp, x2, next_ln[0], next_ln[1], None, bias=b2, res=x1, ldr=hid, y=xn, b_words=weight_x3(w2))
        _stash_ln(x2, next_ln[0], next_ln[1], xn, mn, rn)
    else:
        x2 = linear_fwd(a, w2, b2, prec, res=x1)
    return x2, BlockActs(y1, m1, r1, qkv, att, lse, x1, y2, m2, r2, u, a, None, None, None, None)


WT_MAX_ROWS = 512     # the two operand forms are measured, and held bit for bit, at the small-M tile rules only (csrc/gemm_bf16.hip)


def _dgrad_operand(w, M):
    """(B, b_kn) of the data gradient dx[M, in] = dy . w on bf16-stored operands: the transposed twin in the forward kernel form
    where a current one exists (M <= WT_MAX_ROWS: above, the forms take different tiles and K slabs, and no tile was measured for
    the forward form), else the bf16 shadow read as the [K, N] operand"""
    wt = weight_bf16_t(w) if M <= WT_MAX_ROWS else None
    return (wt, False) if wt is not None else (weight_bf16(w), True)


def _dgrad_bf16(dyb, w, **out):
    """dx[M, in] = dyb[M, out] . w on bf16-stored operands, into C= / Cb= through gemm_bf16's epilogue: on the transposed twin of w in
    the forward kernel form where the fused optimizer epilogue keeps one current, else w [out, in] read as the [K, N] operand; same bits"""
    wo, bkn = _dgrad_operand(w, dyb.shape[0])
    gemm_bf16(dyb, wo, dyb.shape[0], w.shape[1], w.shape[0], b_kn=bkn, **out)


def _dgrad_ln_bwd(route, x3ride, dy, dyb, w, prec, x, nw, nb, mean, rstd, dres, host, *ahead):
    """The data gradient of Linear `w` run into the backward of the LayerNorm (nw, nb) in front of it: (dx, grad_nw, grad_nb, the
    bf16 twin of dx or None).  fast: on bf16 twins, the LayerNorm kernel sums the K slabs of the GEMM itself and prefetches `ahead`
    as `host`; x3ride: the same on fp32 operands with the word shadow of w; else the two launches"""
    (M, N), K = x.shape, w.shape[0]
    if route.fast:
        dxb = bf16_like(x)
        wo, bkn = _dgrad_operand(w, M)
        return gemm_ln_bwd_params(dyb, wo, M, N, K, x, nw, nb, mean, rstd, dres=dres, dx_bf16=dxb,
                                  pf=_prefetch(host, *ahead, dgrad=M), b_kn=bkn) + (dxb,)
    if x3ride:
        return gemm_ln_bwd_params(dy, w, M, N, K, x, nw, nb, mean, rstd, dres=dres, b_words=weight_x3(w)) + (None,)
    return layernorm_bwd_params(linear_dgrad(dy, w, prec), x, nw, nb, mean, rstd, dres=dres) + (None,)


class TransformerBlockFn(torch.autograd.Function):
    """MONAI TransformerBlock: x + attn(norm1(x)); then + mlp(norm2(.)).  ``ckpt`` = activation checkpointing
    (BASELINE.json config[3]): only the block input is kept and backward recomputes the block's forward kernels first."""

    @staticmethod
    def forward(ctx, x, n1w, n1b, wqkv, wp, bp, n2w, n2b, w1, b1, w2, b2, B, L, heads, prec, ckpt=False, next_n1w=None, next_n1b=None,
                emit_twin=False, next_wqkv=None, below_w2=None, below_w1=None):
        """next_n1w / next_n1b: weight and bias of the LayerNorm the NEXT block starts with (not differentiated here: that block
        owns its backward) -- its forward is formed by this block's last kernel.  next_wqkv, below_w2 / below_w1 (detached, prefetch
        only): the qkv weight of the next block, read ahead by that kernel, and linear2 / linear1 of the block BELOW, whose
        backward starts with those two GEMMs right after this block's last backward launch"""
        _require_gpu(x)
        x = _carry_ln(x, x.contiguous())
        train = any(ctx.needs_input_grad[:12])
        ctx.route = _block_route(prec, x.shape[0], x.shape[1], w1.shape[0], x.shape[1] // heads)
        x2, acts = _tblock_forward(x, n1w, n1b, wqkv, wp, bp, n2w, n2b, w1, b1, w2, b2, B, L, heads, prec, ctx.route,
                                   train and not ckpt, None if next_n1w is None else (next_n1w, next_n1b), bool(emit_twin), next_wqkv)
        ctx.below = (below_w2, below_w1)
        ctx.ckpt = bool(ckpt) and train
        ctx.save_for_backward(x, n1w, wqkv, wp, n2w, w1, w2, n1b, bp, n2b, b1, b2, *(() if ctx.ckpt else acts))
        ctx.meta = (B, L, heads, x.shape[1] // heads, prec)
        return x2

    @staticmethod
    def backward(ctx, dx2):
        x, n1w, wqkv, wp, n2w, w1, w2, n1b, bp, n2b, b1, b2, *acts = ctx.saved_tensors
        B, L, heads, dh, prec = ctx.meta
        route = ctx.route
        if ctx.ckpt:
            _, A = _tblock_forward(x, n1w, n1b, wqkv, wp, bp, n2w, n2b, w1, b1, w2, b2, B, L, heads, prec, route, True)
        else:
            A = BlockActs(*acts)
        M, hid = x.shape
        dx2 = dx2.contiguous()
        mlp = w1.shape[0]
        # MLP
        du = dub = dx2b = None
        if route.fast:
            dx2b = _twin(dx2)
            # (du exists as bf16 only: the weight gradient of linear1 is formed from these bf16 values, and so is its bias gradient
            # -- the fp32 copy was 5.3 MB written and read back per block for the column sum alone)
            dub = torch.empty(M, mlp, dtype=torch.bfloat16, device=x.device)
            _dgrad_bf16(dx2b, w2, Cb=dub, act=2, aux=A.u, ldaux=mlp)
        else:
            du = linear_dgrad(dx2, w2, prec, aux=A.u)
        dw2 = wgrad_or_defer(dx2, A.a, prec, w2, dx2b, A.ab)
        db2 = colsum_or_defer(dx2, M, hid, hid, b2)
        dw1 = wgrad_or_defer(du, A.y2, prec, w1, dub, A.y2b)
        db1 = colsum_or_defer(dub if route.fast else du, M, mlp, mlp, b1)
        dx1, dn2w, dn2b, dx1b = _dgrad_ln_bwd(route, route.x3ride, du, dub, w1, prec, A.x1, n2w, n2b, A.m2, A.r2, dx2, "ln2_bwd", wp)
        # attention
        datt = dattb = dqkv = dqkvb = None
        if route.fast:
            if route.b16att:
                dattb = bf16_like(x)
            else:
                datt = torch.empty(M, hid, dtype=torch.float32, device=x.device)
            _dgrad_bf16(dx1b, wp, C=datt, Cb=dattb)
        else:
            datt = linear_dgrad(dx1, wp, prec)
        dwp = wgrad_or_defer(dx1, A.att, prec, wp, dx1b, A.attb)
        dbp = colsum_or_defer(dx1, M, hid, hid, bp)
        if route.b16att:
            dqkvb = attention_bf16_bwd(A.qkv, A.attb, dattb, A.lse, B, L, heads, dh, pf=_prefetch("attn_bwd", wqkv, dgrad=M))
        else:
            dqkvb = torch.empty(M, 3 * hid, dtype=torch.bfloat16, device=x.device) if route.fast else None
            dqkv = attention_bwd(A.qkv, A.att, datt, A.lse, B, L, heads, dh, prec, dqkv_bf16=dqkvb)
        dwqkv = wgrad_or_defer(dqkv, A.y1, prec, wqkv, dqkvb, A.y1b)
        dx, dn1w, dn1b, dxb = _dgrad_ln_bwd(route, route.x3ride_qkv, dqkv, dqkvb, wqkv, prec, x, n1w, n1b, A.m1, A.r1, dx1, "ln1_bwd", *ctx.below)
        if dxb is not None:
            _attach_twin(dx, dxb)      # the block below picks its bf16 operand up from here (functional._twin)
        return (dx, dn1w, dn1b, dwqkv, dwp, dbp, dn2w, dn2b, dw1, db1, dw2, db2) + (None,) * 11


class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, twin=False, below_w2=None, below_w1=None):
        """below_w2 / below_w1 (detached, prefetch only): linear2 / linear1 of the transformer block whose backward follows this
        LayerNorm's (TransformerBlockFn.forward)"""
        _require_gpu(x)
        x = x.contiguous()
        yb = bf16_like(x) if twin else None       # (twin: decoder5's transposed conv reads bf16 tokens in its GEMM form)
        y, mean, rstd = layernorm_fwd(x, w, b, bf16_out=yb)
        if yb is not None:
            _attach_twin(y, yb)
        ctx.save_for_backward(x, w, mean, rstd, b)
        ctx.twin = bool(twin)
        ctx.below = (below_w2, below_w1) if twin else (None, None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, mean, rstd, b = ctx.saved_tensors
        dxb = bf16_like(x) if ctx.twin else None    # bf16 operand for the last transformer block's backward GEMMs
        dx, dw, db = layernorm_bwd_params(dy.contiguous(), x, w, b, mean, rstd, dx_bf16=dxb, pf=_prefetch("ln1_bwd", *ctx.below, dgrad=x.numel() // x.shape[-1]))
        if dxb is not None:
            _attach_twin(dx, dxb)
        return dx, dw, db, None, None, None


# ------------------------------------------------------------------------------ conv-side building blocks
def skip_half(dims, C, prec, device):
    """A fresh concatenation buffer [B,D,H,W,2C] for UnetrUpBlock's torch.cat((up, skip), dim=1), and the view of its second
    half: the producer of the skip tensor writes there directly (``to_cat``) and UpBlockFn(skip_in_cat=True) writes the
    transposed conv into the first half -- the concatenation then costs nothing (it was a 113 MB copy at 96^3)."""
    cat = torch.empty(*dims, 2 * C, dtype=act_dtype(prec), device=device)
    return cat, cat[..., C:]


def cat_of_skip(skip, C):
    """the whole concatenation buffer whose second half ``skip`` is (see skip_half); raises when it is not such a view"""
    B, D, H, W, c = skip.shape
    want = (D * H * W * 2 * C, H * W * 2 * C, W * 2 * C, 2 * C, 1)
    if c != C or tuple(skip.stride()) != want or skip.storage_offset() != C or skip.untyped_storage().nbytes() != B * want[0] * skip.element_size():
        raise RuntimeError("skip_in_cat=True needs the second half of a buffer made by functional.skip_half")
    return skip.as_strided((B, D, H, W, 2 * C), want, 0)


# One record per direction, whatever the route (tests/test_conv_routes_cpu.py pins the launches of every route):
# out: the block's result -- the LOGITS [B, Cout, D, H, W] when `folded`, i.e. the block end went into the out conv's kernel and was
# never stored (otherwise the caller applies the out conv itself); saved = (c1, s1, a1, c2, s2, c3 or None, s3).
BlockFwd = collections.namedtuple("BlockFwd", "out saved folded")
# q1 / q2: the reductions of (dw1, dw3) / dw2 were queued on the arena; dwo, dbo: None unless the head was folded in.
BlockBwd = collections.namedtuple("BlockBwd", "dx dw1 dw2 dw3 q1 q2 dwo dbo")


def _conv3_stats(x, ldx, w, dims, cout, prec):
    """(c, stats) of the 3x3x3 conv with its InstanceNorm statistics: one launch, or conv + statistics pass where that declines"""
    f = conv3_fused(x, ldx, w, None, dims, prec)
    if f is not None:
        return f[0], f[1]
    c = conv3(x, ldx, w, dims, prec)
    return c, instnorm_stats(c, cout, dims[0], dims[1] * dims[2] * dims[3], cout)


def _conv1_generic(x, ldx, w3, dims, cin, cout, prec):
    """the 1x1x1 branch as a stored tensor on the generic GEMM family (fallback of conv3_fused and of the image form)"""
    B, D, H, W = dims
    x32, l32 = _f32_rows(x, ldx, cin)
    c3 = torch.empty(B, D, H, W, cout, dtype=torch.float32, device=x.device)
    gemm(x32, w3, c3, B * D * H * W, cout, cin, lda=l32, ldb=cin, ldc=cout, prec=prec)
    return _act_rows(c3, prec)


def _resblock_fwd(x, ldx, dims, cin, cout, w1, w2, w3, prec, to_cat=False, head=None):
    """MONAI UnetResBlock (instance norm, in != out): lrelu(IN(conv2(lrelu(IN(conv1 x)))) + IN(conv3 x)) -> BlockFwd.
    head = (wo, bo) of the out conv that is the block's only consumer."""
    B, D, H, W = dims
    V = D * H * W
    if in_fuse_level() & 1:
        r = _resblock_fwd_fin(x, ldx, dims, cout, w1, w2, w3, prec, to_cat, head if out_fuse_enabled() else None)
        if r is not None:
            return r
    f1 = conv3_fused(x, ldx, w1, w3, dims, prec)
    if f1 is not None:
        c1, s1, c3, s3 = f1
    else:
        c1, s1 = _conv3_stats(x, ldx, w1, dims, cout, prec)
        c3 = _conv1_generic(x, ldx, w3, dims, cin, cout, prec)
        s3 = instnorm_stats(c3, cout, B, V, cout)
    a1 = instnorm_apply(c1, s1, B, V, cout, True)
    c2, s2 = _conv3_stats(a1, cout, w2, dims, cout, prec)
    half = skip_half(dims, cout, prec, x.device)[1] if to_cat else None
    out = instnorm_apply(c2, s2, B, V, cout, True, x2=c3, sb=s3, out=half, ldo=2 * cout if to_cat else None)
    return BlockFwd(out, (c1, s1, a1, c2, s2, c3, s3), False)


def _resblock_fwd_fin(x, ldx, dims, cout, w1, w2, w3, prec, to_cat, head=None):
    """the same block in FOUR launches: both convs leave their InstanceNorm sums as partial rows and the two apply kernels form
    the statistics in their prologues (no finalize launches); None when a shape declines (the caller takes the route above).
    head = (wo, bo): the block end goes into the out conv's kernel when that accepts the shape."""
    B, D, H, W = dims
    V = D * H * W
    cin = w1.shape[1]
    # the block on the image (<= 4 fp32 input channels, no input gradient): its 1x1x1 branch is never stored -- the block-end
    # kernels form it from the image (csrc/norm_misc.hip: ImgBranch)
    img = (x.dtype == torch.float32 and cin <= 4 and ldx == cin and not x.requires_grad and w3.is_contiguous()
           and cout % 8 == 0 and 64 % max(1, cout // 8) == 0)
    f1 = conv3_parts(x, ldx, w1, w3, dims, prec, store3=not img)
    if f1 is None and img:
        img = False
        f1 = conv3_parts(x, ldx, w1, w3, dims, prec)
    if f1 is None:
        return None
    c1, p1, c3, p3, rows1 = f1
    r1 = instnorm_apply_fin(c1, p1, rows1, B, V, cout, True)
    if r1 is None:
        return None
    a1, s1, _ = r1
    f2 = conv3_parts(a1, cout, w2, None, dims, prec)
    if f2 is None:
        return None
    c2, p2, _, _, rows2 = f2
    if head is not None and not img and not to_cat:
        r = outconv_in_fwd(c2, p2, rows2, c3, p3, rows1, head[0], head[1], B, V, cout)
        if r is not None:
            return BlockFwd(r[0].view(B, head[0].shape[0], D, H, W), (c1, s1, a1, c2, r[1], c3, r[2]), True)
    half = skip_half(dims, cout, prec, x.device)[1] if to_cat else None
    r2 = instnorm_apply_fin_img(c2, p2, rows2, x, cin, w3, p3, rows1, B, V, cout, out=half, ldo=2 * cout if to_cat else None) if img else None
    if r2 is None:
        if img:                                # (a shape the image form declines: materialise the branch after all)
            c3 = _conv1_generic(x, ldx, w3, dims, cin, cout, prec)
        r2 = instnorm_apply_fin(c2, p2, rows2, B, V, cout, True, x2=c3, part_b=p3, rows_b=rows1, out=half, ldo=2 * cout if to_cat else None)
    if r2 is None:
        return None
    out, s2, s3 = r2
    return BlockFwd(out, (c1, s1, a1, c2, s2, c3, s3), False)


def _resblock_bwd(dout, x, ldx, dims, cin, cout, w1, w2, w3, saved, prec, need_dx, head=None):
    """-> BlockBwd.  head = (wo, bo): the block end was folded into the out conv (the forward's record says `folded`): ``dout`` is
    the gradient of the LOGITS."""
    B, D, H, W = dims
    V = D * H * W
    c1, s1, a1, c2, s2, c3, s3 = saved
    dwo = dbo = img_rows = None

    def stored(dout, lddo, c3):
        return instnorm_bwd(dout, lddo, c2, s2, B, V, cout, True, x2=c3, sb=s3)
    # the gradient at the block end: dc2, dc3 -- or, from the image form, partial rows of dw3 in the place of dc3
    if head is not None:
        # folded head: the out conv's backward leaves the InstanceNorm backward sums as partial rows
        dout, hpart, hrows, dwo, dbo = outconv_in_bwd(dout, c2, s2, c3, s3, head[0], head[1], B, V, cout)
        ends = instnorm_bwd_apply_fin_dual(dout, cout, c2, s2, c3, s3, hpart, hrows, B, V, cout)
        if ends is None:                       # fallback: the stored form's reduction pass over the out conv's data gradient
            ends = stored(*_rows(dout), c3)
        dc2, dc3 = ends
    elif c3 is None:
        # the block on the image: the 1x1x1 branch was never stored -- its gradient is formed per voxel inside the backward apply and
        # leaves only as partial rows of dw3
        dout, lddo = _rows(dout)
        img = instnorm_bwd_img(dout, lddo, c2, s2, x, cin, w3, s3, B, V, cout)
        if img is None:                        # fallback: materialise the branch and take the stored form
            dc2, dc3 = stored(dout, lddo, _conv1_generic(x, ldx, w3, dims, cin, cout, prec))
        else:
            dc2, dc3, img_rows = img[0], None, img[1:]
    else:
        dc2, dc3 = stored(*_rows(dout), c3)
    # arena mode: the three weight gradients' partial-sum reductions join the grouped launch at the end of the backward pass
    st, (g1, g2, g3) = grad_arena.dests(w1, w2, w3)
    # conv3 (1x1x1)
    dw3 = g3 if g3 is not None else torch.empty(cout, cin, 1, 1, 1, dtype=torch.float32, device=x.device)
    # conv2
    dw2, q2 = _conv3_wgrad_queued(st, a1, cout, dc2, cout, dims, cout, cout, prec, out=g2)
    dc1 = None
    if in_fuse_level() & 2:
        # the backward sums of the first norm come out of the data-gradient conv's epilogue: no reduction pass over (da1, c1)
        f = conv3_dgrad_stats(dc2, w2, c1, s1, dims, prec)
        if f is not None:
            da1, bpart, brows = f
            dc1 = instnorm_bwd_apply_fin(da1, cout, c1, s1, bpart, brows, 2, B, V, cout, True)
    if dc1 is None:
        da1 = conv3(dc2, cout, w2, dims, prec, mode=1)
        dc1, _ = instnorm_bwd(da1, cout, c1, s1, B, V, cout, True)
    dw1, q1 = _conv3_wgrad_queued(st, x, ldx, dc1, cout, dims, cin, cout, prec, out=g1, dy3=dc3, out3=dw3 if dc3 is not None else None)
    if img_rows is not None:
        rq = (img_rows[0], dw3, cout * cin, img_rows[1])
        if q1:
            st.queue_reduce(*rq)           # joins the grouped reduce at the end of the backward pass
        else:
            grad_arena.launch_reduces([rq])
    dx = None
    if need_dx:
        dx = torch.empty(B, D, H, W, cin, dtype=act_dtype(prec), device=x.device)
        if not conv3_dgrad_fused(dc1, dc3, w1, w3, dx, dims, prec):
            # two kernels: the 1x1x1 data gradient on the generic GEMM family, and the 3x3x3 one accumulates onto it
            d32 = torch.empty(B, D, H, W, cin, dtype=torch.float32, device=x.device)
            dc3_32, ld3 = _f32_rows(dc3, cout, cout)
            gemm(dc3_32, w3, d32, B * V, cin, cout, lda=ld3, ldb=cin, ldc=cin, prec=prec, b_trans=True)
            _act_rows(d32, prec, out=dx)
            conv3(dc1, cout, w1, dims, prec, mode=1, out=dx, ldo=cin, accumulate=True)
    return BlockBwd(dx, dw1, dw2, dw3, q1, q2, dwo, dbo)


class ResBlockFn(torch.autograd.Function):
    """UnetrBasicBlock(res_block=True) = one UnetResBlock (encoder1, unetr.py:90-98)."""

    @staticmethod
    def forward(ctx, x, w1, w2, w3, prec, to_cat=False):
        """to_cat: the result is the second half of a fresh concatenation buffer (functional.skip_half)"""
        _require_gpu(x, act=True)
        x, ldx = _rows(x)
        B, D, H, W, cin = x.shape
        cout = w1.shape[0]
        r = _resblock_fwd(x, ldx, (B, D, H, W), cin, cout, w1, w2, w3, prec, to_cat)
        ctx.save_for_backward(x, w1, w2, w3, *r.saved)
        ctx.meta = (ldx, (B, D, H, W), cin, cout, prec)
        return r.out

    @staticmethod
    def backward(ctx, dout):
        x, w1, w2, w3, *saved = ctx.saved_tensors
        ldx, dims, cin, cout, prec = ctx.meta
        g = _resblock_bwd(dout, x, ldx, dims, cin, cout, w1, w2, w3, saved, prec, ctx.needs_input_grad[0])
        return g.dx, _ret(w1, g.dw1, deferred=g.q1), _ret(w2, g.dw2, deferred=g.q2), _ret(w3, g.dw3, deferred=g.q1), None, None


class TconvFn(torch.autograd.Function):
    """2x2x2 stride-2 ConvTranspose3d, bias=False (UnetrPrUpBlock with conv_block=False, unetr.py:99-134)."""

    @staticmethod
    def forward(ctx, x, w, prec, to_cat=False):
        """to_cat: the result is the second half of a fresh concatenation buffer (functional.skip_half)"""
        _require_gpu(x, act=True)
        x, ldx = _rows(x)
        B, D, H, W, cin = x.shape
        cout = w.shape[1]
        half = skip_half((B, 2 * D, 2 * H, 2 * W), cout, prec, x.device)[1] if to_cat else None
        y, xb = tconv_fwd(x, ldx, w, (B, D, H, W), cin, cout, prec, out=half, ldo=2 * cout if to_cat else None)
        ctx.save_for_backward(x, w)
        ctx.xb = xb
        ctx.meta = (ldx, (B, D, H, W), cin, cout, prec)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        ldx, dims, cin, cout, prec = ctx.meta
        dy, lddy = _rows(dy)
        dx, dw = tconv_bwd(x, ldx, ctx.xb, dy, lddy, w, dims, cin, cout, prec, ctx.needs_input_grad[0])
        return dx, dw, None, None


def _outconv_fwd(x, ldx, w, b):
    B, D, H, W, cin = x.shape
    cout = w.shape[0]
    logits = torch.empty(B, cout, D, H, W, dtype=torch.float32, device=x.device)
    call("unetr_outconv_fwd", x.data_ptr(), ldx, w.data_ptr(), b.data_ptr(), logits.data_ptr(), B, D * H * W, cin, cout, _a16(x), _stream())
    return logits


def _outconv_bwd(dl, x, ldx, w, b):
    B, D, H, W, cin = x.shape
    cout = w.shape[0]
    dl = dl.contiguous()
    dx = torch.empty(B, D, H, W, cin, dtype=x.dtype, device=x.device)
    gw, gb = _gout(w), _gout(b)
    dw = gw if gw is not None else torch.empty_like(w)
    db = gb if gb is not None else torch.empty(cout, dtype=torch.float32, device=x.device)
    ws = workspace(x.device)
    call("unetr_outconv_bwd", dl.data_ptr(), x.data_ptr(), ldx, w.data_ptr(), dx.data_ptr(), cin, dw.data_ptr(), db.data_ptr(),
         B, D * H * W, cin, cout, ws.data_ptr(), ws.numel() * 4, _a16(x), _stream())
    return dx, dw, db


class UpBlockFn(torch.autograd.Function):
    """MONAI UnetrUpBlock(res_block=True): tconv(inp) -> cat(up, skip) -> UnetResBlock (unetr.py:135-174).
    The transposed conv writes straight into the first half of the concatenation buffer.
    With (wo, bo) -- the weights of the UnetOutBlock that is this block's only consumer (decoder2 -> out, unetr.py:165-175,206-207)
    -- the Function returns the LOGITS: the block end lrelu(IN(c2) + IN(c3)) is formed inside the out conv's kernels and never
    stored (forward: one tensor write + one read fewer; backward: the InstanceNorm backward reduction pass disappears)."""

    @staticmethod
    def forward(ctx, inp, skip, wt, w1, w2, w3, prec, skip_in_cat=False, wo=None, bo=None):
        """skip_in_cat: ``skip`` already is the second half of a concatenation buffer made by functional.skip_half (its
        producer ran with to_cat=True): no copy"""
        _require_gpu(inp, act=True)
        inp, ldi = _rows(inp)
        B, D, H, W, cin = inp.shape
        C = wt.shape[1]
        dims2 = (B, 2 * D, 2 * H, 2 * W)
        in_cat = skip_in_cat and skip.dtype == act_dtype(prec)
        cat = cat_of_skip(skip, C) if in_cat else torch.empty(*dims2, 2 * C, dtype=act_dtype(prec), device=inp.device)
        _, ctx.xb = tconv_fwd(inp, ldi, wt, (B, D, H, W), cin, C, prec, out=cat, ldo=2 * C)
        if not in_cat:
            skip, lds = _rows(_as_act(skip, prec))
            call("unetr_copy_rows", cat.data_ptr() + cat.element_size() * C, 2 * C, skip.data_ptr(), lds, B * 8 * D * H * W, C, 0, _a16(cat), _stream())
        ctx.meta = (ldi, (B, D, H, W), cin, C, prec)
        r = _resblock_fwd(cat, 2 * C, dims2, 2 * C, C, w1, w2, w3, prec, head=(wo, bo) if wo is not None else None)
        ctx.head_folded = r.folded          # (a head exists where wo is saved; where it was not folded in, the out conv runs on its own)
        stored_end = r.out if wo is not None and not r.folded else None
        ctx.save_for_backward(inp, wt, w1, w2, w3, cat, wo, bo, stored_end, *r.saved)
        return r.out if stored_end is None else _outconv_fwd(stored_end, C, wo, bo)

    @staticmethod
    def backward(ctx, dout):
        ldi, dims, cin, C, prec = ctx.meta
        B, D, H, W = dims
        dims2 = (B, 2 * D, 2 * H, 2 * W)
        inp, wt, w1, w2, w3, cat, wo, bo, stored_end, *saved = ctx.saved_tensors
        if stored_end is not None:
            dout, dwo, dbo = _outconv_bwd(dout, stored_end, C, wo, bo)
        g = _resblock_bwd(dout, cat, 2 * C, dims2, 2 * C, C, w1, w2, w3, saved, prec, True, head=(wo, bo) if ctx.head_folded else None)
        if stored_end is None:
            dwo, dbo = g.dwo, g.dbo         # (None without a head)
        head_ret = (_ret(wo, dwo), _ret(bo, dbo)) if wo is not None else (None, None)
        dcat = g.dx
        dinp, dwt = tconv_bwd(inp, ldi, ctx.xb, dcat, 2 * C, wt, dims, cin, C, prec, ctx.needs_input_grad[0])
        dskip = dcat[..., C:] if ctx.needs_input_grad[1] else None
        return (dinp, dskip, dwt, _ret(w1, g.dw1, deferred=g.q1), _ret(w2, g.dw2, deferred=g.q2), _ret(w3, g.dw3, deferred=g.q1), None, None) + head_ret


class OutConvFn(torch.autograd.Function):
    """MONAI UnetOutBlock: 1x1x1 conv with bias; emits NCDHW logits (unetr.py:175,207)."""

    @staticmethod
    def forward(ctx, x, w, b):
        _require_gpu(x, act=True)
        x, ldx = _rows(x)
        ctx.save_for_backward(x, w, b)
        ctx.ldx = ldx
        return _outconv_fwd(x, ldx, w, b)

    @staticmethod
    def backward(ctx, dl):
        x, w, b = ctx.saved_tensors
        dx, dw, db = _outconv_bwd(dl, x, ctx.ldx, w, b)
        return dx, _ret(w, dw), _ret(b, db)


class ToNCDHWFn(torch.autograd.Function):
    """channels-last [B,D,H,W,C] -> torch NCDHW [B,C,D,H,W] (the layout enc4 is returned in, unetr.py:208)."""

    @staticmethod
    def forward(ctx, x):
        _require_gpu(x, act=True)
        x, ldx = _rows(x)
        B, D, H, W, C = x.shape
        y = torch.empty(B, C, D, H, W, dtype=torch.float32, device=x.device)
        call("unetr_nhwc_to_nchw", x.data_ptr(), ldx, y.data_ptr(), B, C, D * H * W, 0, _a16(x), _stream())
        ctx.adt = x.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        B, C, D, H, W = dy.shape
        dx = torch.empty(B, D, H, W, C, dtype=ctx.adt, device=dy.device)
        call("unetr_nchw_to_nhwc", dy.data_ptr(), dx.data_ptr(), C, B, C, D * H * W, _a16(dx), _stream())
        return dx


def to_channels_last(x_in):
    """NCDHW image -> channels-last (no gradient: the image is a leaf input). C == 1 is a free view."""
    _require_gpu(x_in)
    B, C, D, H, W = x_in.shape
    x_in = x_in.contiguous()
    if C == 1:
        return x_in.view(B, D, H, W, 1)
    y = torch.empty(B, D, H, W, C, dtype=torch.float32, device=x_in.device)      # (the image stays fp32 in every mode)
    call("unetr_nchw_to_nhwc", x_in.data_ptr(), y.data_ptr(), C, B, C, D * H * W, 0, _stream())
    return y


def _loss_inputs(logits, label, multilabel):
    """forward prologue of the per-voxel loss Functions -> (logits, label, B, C, V): contiguous fp32 device logits [B,C,*spatial] and
    the label as contiguous fp32, class ids [B,1,*spatial] or, multilabel, a mask shaped like the logits"""
    _require_gpu(logits)
    logits = logits.contiguous()
    label = label.contiguous().to(torch.float32)
    B, C = logits.shape[0], logits.shape[1]
    V = logits.numel() // (B * C)
    if multilabel and label.numel() != B * C * V:
        raise ValueError(f"multi-label target must be [B,C,*spatial] like the logits, got {tuple(label.shape)}")
    if not multilabel and label.numel() != B * V:
        raise ValueError(f"label must be [B,1,*spatial] class indices, got {tuple(label.shape)}")
    return logits, label, B, C, V


class DiceCEFn(torch.autograd.Function):
    """DiceCELoss -> (loss, dice, ce) as a 3-vector.  multilabel=False: DiceCELoss(to_onehot_y=True, softmax=True)
    (unetr_segmentation_3d.py:404); multilabel=True: DiceCELoss(to_onehot_y=False, sigmoid=True) (:477-482)."""

    @staticmethod
    def forward(ctx, logits, label, smooth_nr, smooth_dr, multilabel=False, scalar=False):
        """scalar=True: returns the 0-dim loss itself (what DiceCELoss.forward hands to backward()): selecting element 0 of the
        3-vector through autograd cost a fill, a zero and a copy launch in every backward pass"""
        logits, label, B, C, V = _loss_inputs(logits, label, multilabel)
        out = torch.empty(3, dtype=torch.float32, device=logits.device)
        coef = torch.empty(B * C * 2, dtype=torch.float32, device=logits.device)
        ws = workspace(logits.device)
        call("unetr_dicece_fwd", logits.data_ptr(), label.data_ptr(), B, C, V, int(multilabel), smooth_nr, smooth_dr, out.data_ptr(),
             coef.data_ptr(), ws.data_ptr(), ws.numel() * 4, _stream())
        ctx.save_for_backward(logits, label, coef)
        ctx.meta = (B, C, V, int(multilabel))
        ctx.scalar = bool(scalar)
        return out[0] if scalar else out

    @staticmethod
    def backward(ctx, dout):
        logits, label, coef = ctx.saved_tensors
        B, C, V, ml = ctx.meta
        # only out[0] (= dice + ce) is differentiable; out[1], out[2] are reporting copies
        dloss = dout.reshape(1) if ctx.scalar else dout[0:1]
        dloss = dloss.contiguous()
        dlogits = torch.empty_like(logits)
        call("unetr_dicece_bwd", logits.data_ptr(), label.data_ptr(), coef.data_ptr(), dloss.data_ptr(), dlogits.data_ptr(), B, C, V,
             ml, _stream())
        return dlogits, None, None, None, None, None


class SegLossFn(torch.autograd.Function):
    """The segmentation loss family of csrc/seg_loss.hip -> (loss, region term, voxel term) as a 3-vector.  `cfg` holds the fields of
    unetr_segloss_desc that do not depend on the input (seg_losses.SegLoss builds it); `class_weight` is a device tensor [C] or None."""

    @staticmethod
    def _desc(cfg, B, C, V, class_weight):
        d = _capi.SegLossDesc(B=B, C=C, V=V, **cfg)
        d.class_weight = class_weight.data_ptr() if class_weight is not None else None
        return d

    @staticmethod
    def forward(ctx, logits, label, cfg, class_weight=None, scalar=False):
        """scalar=True: returns the 0-dim loss itself, as DiceCEFn does"""
        logits, label, B, C, V = _loss_inputs(logits, label, cfg["multilabel"])
        if not cfg["include_background"] and C == 1:
            raise ValueError("include_background=False needs more than one channel")
        if class_weight is not None and class_weight.numel() != C:
            raise ValueError(f"class_weight has {class_weight.numel()} entries for {C} channels")
        d = SegLossFn._desc(cfg, B, C, V, class_weight)
        out = torch.empty(3, dtype=torch.float32, device=logits.device)
        coef = torch.empty(B * C * 3 + 1, dtype=torch.float32, device=logits.device)
        ws = workspace(logits.device)
        call("unetr_segloss_fwd", ctypes.byref(d), logits.data_ptr(), label.data_ptr(), out.data_ptr(), coef.data_ptr(), ws.data_ptr(),
             ws.numel() * 4, _stream())
        ctx.save_for_backward(logits, label, coef)
        ctx.desc, ctx.class_weight = d, class_weight            # (the tensor is kept alive with the pointer the descriptor holds)
        ctx.scalar = bool(scalar)
        return out[0] if scalar else out

    @staticmethod
    def backward(ctx, dout):
        logits, label, coef = ctx.saved_tensors
        # only out[0] is differentiable; out[1], out[2] are reporting copies
        dloss = dout.reshape(1) if ctx.scalar else dout[0:1]
        dloss = dloss.contiguous()
        dlogits = torch.empty_like(logits)
        call("unetr_segloss_bwd", ctypes.byref(ctx.desc), logits.data_ptr(), label.data_ptr(), coef.data_ptr(), dloss.data_ptr(),
             dlogits.data_ptr(), _stream())
        return dlogits, None, None, None, None
