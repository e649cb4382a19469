"""Arena gradients: parameters registered here get their gradients written straight into a slice of one flat arena
(UNETR.use_flat_buffers), so AdamW is one launch and the data-parallel all-reduce needs no flatten copies.

Everything mutable about that fast path -- the sink table, the queue of work deferred to the end of the backward pass, the
readiness callbacks of the data-parallel reducer -- belongs to ONE ArenaState per model (UNETR.use_flat_buffers creates it),
so several models in one process do not share a queue.  The module-level table only maps a parameter's storage address to
its owner; entries are validated against the live parameter (weak reference + address) on every lookup.

Deferred work: weight / bias gradients that nothing inside backward needs are queued on the owning state (queue_wgrad,
queue_wgrad_bf16, queue_colsum, queue_reduce -- the only way in) and launched by ONE autograd end-of-pass callback
(flush_deferred) as a few grouped kernels instead of ~90 small latency-bound launches.

functional.py imports this module and fills in the three hooks below; nothing here imports functional.
"""
import ctypes
import weakref

import torch

from . import _capi
from ._capi import call

# hooks set by functional.py
_stream = None        # () -> id of the current stream
_drop_twins = None    # (flat): forget a model's transposed-twin arena and the table entries that point into it
_twin_arena = None    # (flat) -> the transposed-twin arena the fused AdamW epilogue writes too, or None (UNETR_AMD_WT, read per flush)


class _Deferred:
    """what one backward pass has queued for its end"""
    __slots__ = ("reduce", "wgrad_bf16", "wgrad", "colsum", "params", "armed")

    def __init__(self):
        self.reduce = []        # (part, dst, n, rows): dst[i] = sum over rows of part[row][i]
        self.wgrad_bf16 = []    # (dyb, xb, out): out[N,K] = dyb[M,N]^T xb[M,K], bf16-stored operands
        self.wgrad = []         # (dy, x, out, prec): the same with fp32-stored operands
        self.colsum = []        # (x, out, M, N, ld): out[N] = column sums of x[M,N], row pitch ld
        self.params = []        # parameters whose readiness callbacks wait for the launches
        self.armed = False      # the end-of-pass callback of this backward pass is queued


class ArenaState:
    def __init__(self):
        self.sinks = {}            # data_ptr -> (weakref(param), arena view)
        self.ready_cb = []         # data-parallel reducers: called with a parameter once its arena gradient is final
        self.deferred = _Deferred()
        self.unmaintained = 0      # arena shadows of THIS model re-derived since its flat optimizer last vouched for them
        self.fuse = None           # optim.AdamW.begin_fused_step: the deferred weight-gradient launch applies AdamW itself
        self.flat = None           # the model's arenas (UNETR.use_flat_buffers)

    def _arm(self):
        q = self.deferred
        if not q.armed:
            q.armed = True
            torch.autograd.Variable._execution_engine.queue_callback(lambda: flush_deferred(self))

    def queue_wgrad(self, dy, x, out, prec):
        """out[N,K] = dy[M,N]^T x[M,K] (fp32 storage, precision mode `prec`) at the end of the backward pass"""
        self.deferred.wgrad.append((dy, x, out, prec))
        self._arm()

    def queue_wgrad_bf16(self, dyb, xb, out):
        """the same from bf16-stored operands; the launch that carries an armed optimizer / communication epilogue (`fuse`)"""
        self.deferred.wgrad_bf16.append((dyb, xb, out))
        self._arm()

    def queue_colsum(self, x, out, M, N, ld):
        """out[N] = column sums of x[M,N] (row pitch ld, fp32 or bf16) at the end of the backward pass"""
        self.deferred.colsum.append((x, out, M, N, ld))
        self._arm()

    def queue_reduce(self, part, dst, n, rows):
        """dst[i] = sum over `rows` partial rows of part[row][i], i < n, at the end of the backward pass"""
        self.deferred.reduce.append((part, dst, n, rows))
        self._arm()

    def reset_deferred(self):
        """Drop whatever a backward pass that raised left queued (its end-of-pass callback never ran): without this the
        queue stays armed, no later pass re-arms the flush, and AdamW steps on stale arena gradients."""
        self.deferred = _Deferred()

    def clear(self):
        self.fuse = None
        _drop_twins(self.flat)
        for k in list(self.sinks):
            _GRAD_SINK.pop(k, None)
        self.sinks.clear()
        self.reset_deferred()


_DEFAULT_STATE = ArenaState()
_GRAD_SINK = {}                    # data_ptr -> ArenaState owning that parameter


def register_grad_sinks(params_and_views, state=None):
    state = state if state is not None else _DEFAULT_STATE
    for p, view in params_and_views:
        state.sinks[p.data_ptr()] = (weakref.ref(p), view)
        _GRAD_SINK[p.data_ptr()] = state
    return state


def clear_grad_sinks(state=None):
    """forget the arena registrations (of one model's state, or of every model when called without one)"""
    if state is not None:
        state.clear()
        return
    for st in set(_GRAD_SINK.values()):
        st.clear()
    _DEFAULT_STATE.clear()
    _GRAD_SINK.clear()


def owner(w):
    """the ArenaState a tensor at the storage address of `w` is registered with, or None"""
    return _GRAD_SINK.get(w.data_ptr())


def _sink(w):
    """(state, param, view) when tensor `w` IS a registered, still-living parameter at its registered address"""
    st = _GRAD_SINK.get(w.data_ptr())
    if st is None:
        return None
    ent = st.sinks.get(w.data_ptr())
    if ent is None:
        return None
    p = ent[0]()
    if p is None or p.data_ptr() != w.data_ptr() or ent[1].shape != w.shape:
        return None
    return st, p, ent[1]


def dest(w):
    """Where the gradient of parameter tensor `w` goes and who owns it: (state, arena slice) when registered and no gradient is
    currently attached (accumulating into an existing .grad must not alias it), else (None, None): a fresh tensor."""
    ent = _sink(w)
    if ent is None or ent[1].grad is not None:
        return None, None
    return ent[0], ent[2]


def dests(*ws):
    """(state, slices) of several parameters whose deferred work is queued together: the state only when every one of them has
    a slice and all are registered with the same state; each slice as dest() gives it"""
    found = [dest(w) for w in ws]
    st = found[0][0]
    if any(s is None or s is not st for s, _ in found):
        st = None
    return st, [g for _, g in found]


def _gout(w):
    return dest(w)[1]


def _ret(w, g, deferred=False):
    """What a Function.backward returns for parameter `w`: when `g` was (or, if deferred, will be) written into
    w's arena slice, attach the slice as .grad directly (autograd would clone it: the arena keeps a second
    reference) and return None.  Readiness callbacks (data-parallel buckets) fire now, or at flush if deferred."""
    ent = _sink(w) if g is not None else None
    if ent is not None and g.data_ptr() == ent[2].data_ptr():
        st, p, view = ent
        p.grad = view
        if deferred:
            st.deferred.params.append(p)
        else:
            for cb in st.ready_cb:
                cb(p)
        return None
    return g


# ---- the grouped launches ---------------------------------------------------------------------------------------------
def _grouped(entries):
    """GroupedProblem array of entries that begin with (dy, x, out): out[N,K] = dy[M,N]^T x[M,K]"""
    arr = (_capi.GroupedProblem * len(entries))()
    for a, (dy, x, out, *_) in zip(arr, entries):
        a.dy, a.x, a.dw = dy.data_ptr(), x.data_ptr(), out.data_ptr()
        a.M, a.N, a.K = dy.shape[0], dy.shape[1], x.shape[1]
    return arr


def launch_reduces(rq):
    """every queued weight-gradient reduction (dst[i] = sum over rows of part[row][i]) in ONE launch"""
    arr = (_capi.ReduceProblem * len(rq))()
    for a, (part, dst, n, rows) in zip(arr, rq):
        a.part, a.dst, a.n, a.rows = part.data_ptr(), dst.data_ptr(), n, rows
    call("unetr_reduce_rows_grouped", arr, len(rq), _stream())


def launch_wgrad_bf16(wbq, fuse=None):
    """The bf16-storage weight gradients (dyb, xb, out) in ONE grouped launch.  With an epilogue armed (`fuse`) the optimizer rides
    on the launch: problems whose destination is a registered arena slice get AdamW -- or, for the data-parallel step, the bf16 cast
    into the communication buffer -- in the epilogue (their gradient is never stored); anything else keeps the plain launch."""
    if fuse is not None:
        index = fuse["index"]
        fused = [q for q in wbq if q[2].data_ptr() in index]
        wbq = [q for q in wbq if q[2].data_ptr() not in index]
        if fused:
            done = [index[q[2].data_ptr()] for q in fused]
            if fuse.get("kind") == "bf16out":      # data-parallel step, bf16 communication: bf16(dW) straight into the comm buffer
                call("unetr_gemm_bf16_grouped_wgrad_bf16out", _grouped(fused), len(fused), fuse["grad"], fuse["out"], fuse["total"], _stream())
            else:
                # (the transposed twins of the weights, if this model keeps them, are written by the same epilogue)
                wt = _twin_arena(fuse.get("flat"))
                call("unetr_gemm_bf16_grouped_wgrad_adamw_t", _grouped(fused), len(fused), ctypes.byref(fuse["arena"]),
                     (ctypes.c_int * len(done))(*done), wt.data_ptr() if wt is not None else None, _stream())
                if wt is not None:
                    fuse["wt_done"].extend(done)
            fuse["done"].extend(done)
    if wbq:
        call("unetr_gemm_bf16_grouped_wgrad", _grouped(wbq), len(wbq), _stream())


def launch_wgrad_x3(wq, fuse=None):
    """bf16x3 weight gradients (dy, x, out, prec): dW = dY^T X over (hi, lo) halves is the bf16 kernel's contraction over three times
    the rows of the stacks [dYh; dYh; dYl] / [Xh; Xl; Xh] (every stack of the pass split in one streaming launch) -- the generic
    fp32-storage grouped kernel spends 2.2 ms per step on these 76 GF, the bf16 kernel 0.2 ms per 432 rows; with an optimizer
    epilogue armed it rides here too.  Returns the entries whose shape or layout the stacks cannot take (generic launch)."""
    rest, stacked, splits = [], [], []
    for ent in wq:
        dy, x, out = ent[:3]
        M, N, K = dy.shape[0], dy.shape[1], x.shape[1]
        if (M * N) % 8 or (M * K) % 8 or (3 * M) % 8 or N % 8 or K % 8 or not dy.is_contiguous() or not x.is_contiguous():
            rest.append(ent)
            continue
        dys = torch.empty(3 * M, N, dtype=torch.bfloat16, device=dy.device)
        xs = torch.empty(3 * M, K, dtype=torch.bfloat16, device=dy.device)
        splits += [(dy, dys, M, N, 0), (x, xs, M, K, 1)]
        stacked.append((dys, xs, out))
    if stacked:
        arr = (_capi.SplitProblem * len(splits))()
        for a, (src, dst, rows, cols, second) in zip(arr, splits):
            a.src, a.dst, a.rows, a.cols, a.second = src.data_ptr(), dst.data_ptr(), rows, cols, second
        call("unetr_split_stack_bf16_grouped", arr, len(splits), _stream())
        launch_wgrad_bf16(stacked, fuse)
    return rest


def launch_wgrad(wq, prec):
    """the fp32-storage weight gradients (dy, x, out, ...) in ONE grouped launch of the generic kernel"""
    call("unetr_gemm_grouped_wgrad", _grouped(wq), len(wq), prec, _stream())


def launch_colsums(cq):
    """the column sums (x, out, M, N, ld) in ONE grouped launch"""
    arr = (_capi.ColsumProblem * len(cq))()
    for a, (x, out, M, N, ld) in zip(arr, cq):
        a.x, a.out, a.ld, a.M, a.N = x.data_ptr(), out.data_ptr(), ld, M, N
        a.x_bf16 = int(x.dtype == torch.bfloat16)
    call("unetr_colsum_grouped", arr, len(cq), _stream())


def flush_deferred(st=None):
    """Runs at the end of the backward pass (autograd engine callback) on the backward stream."""
    st = st if st is not None else _DEFAULT_STATE
    q = st.deferred
    st.reset_deferred()
    wq = q.wgrad
    precs = {ent[3] for ent in wq}
    if len(precs) > 1:
        raise RuntimeError(f"deferred weight gradients of one backward pass were queued in different precision modes: {sorted(precs)}")
    if q.reduce:
        launch_reduces(q.reduce)
    if q.wgrad_bf16:
        launch_wgrad_bf16(q.wgrad_bf16, st.fuse)
    if wq and _capi.PREC_BF16X3 in precs:
        wq = launch_wgrad_x3(wq, st.fuse)
    if wq:
        launch_wgrad(wq, wq[0][3])
    if q.colsum:
        launch_colsums(q.colsum)
    for p in q.params:
        for cb in st.ready_cb:
            cb(p)
