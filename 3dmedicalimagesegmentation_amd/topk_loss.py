"""Exact order statistics on the device and what is built on them: ``kth_value`` and ``percentile`` (csrc/select.hip, a radix
select over the bit pattern of fp32 values: a fixed number of histogram passes, no sort, no index tensor) and nnU-Net's hard-voxel
mining, ``TopKLoss`` -- cross entropy averaged over the k % hardest voxels of the batch -- with ``DiceTopKLoss`` (csrc/topk_loss.hip).
Every call is a fixed sequence of launches on the current stream, without a host synchronisation and with scratch from
``functional.workspace``, so the losses sit inside a captured training step and ``k`` is a device scalar that ``set_k`` may change
between replays.  No CPU fallback."""
import ctypes
import math

import torch
import torch.nn as nn

from . import functional as Fn
from . import loss_common as lc
from ._capi import SELECT_LARGEST, TopKCEDesc, call
from .seg_losses import SegLoss, _activation


def _select(x, n, out_row, rank_host=0, rank_dev=None, largest=False):
    """one unetr_select_kth call on x[0:n] (contiguous fp32 device memory); out_row: three int32 words that receive the result"""
    ws = Fn.workspace(x.device)
    call("unetr_select_kth", x.data_ptr(), n, rank_dev.data_ptr() if rank_dev is not None else None, int(rank_host),
         SELECT_LARGEST if largest else 0, out_row.data_ptr(), ws.data_ptr(), ws.numel() * 4, Fn._stream())


def _check_array(x):
    Fn._require_gpu(x)
    if not x.is_contiguous():
        raise ValueError("a contiguous tensor is expected")
    if not 1 <= x.numel() < 2 ** 31:
        raise ValueError(f"1 <= numel < 2**31 expected, got {x.numel()}")


def kth_value(x: torch.Tensor, k, largest: bool = False) -> torch.Tensor:
    """The k-th smallest (``largest=True``: k-th largest) element of ``x``, k counted from 0, as a 0-dim float32 device tensor:
    ``np.partition(x.ravel(), k)[k]``.  ``k`` is an int, or an int32 device tensor with one element that is read when the kernels
    run.  Order: the total order of the fp32 bit patterns (-0 below +0, NaNs at the ends).  Does not synchronise."""
    _check_array(x)
    n = x.numel()
    res = torch.empty(3, dtype=torch.int32, device=x.device)
    if isinstance(k, torch.Tensor):
        if k.dtype != torch.int32 or k.numel() != 1 or k.device != x.device:
            raise ValueError("a device rank must be one int32 element on the array's device")
        _select(x, n, res, rank_dev=k, largest=largest)
    else:
        if not 0 <= int(k) < n:
            raise ValueError(f"k={k!r}: expected 0 <= k < {n}")
        _select(x, n, res, rank_host=int(k), largest=largest)
    return res[0:1].view(torch.float32)[0]


def select_counts(x: torch.Tensor, k: int, largest: bool = False):
    """(value, n_beyond, n_equal) of ``kth_value`` as device tensors: the elements strictly beyond the value on the selected side, and
    the elements with the value's bits"""
    _check_array(x)
    if not 0 <= int(k) < x.numel():
        raise ValueError(f"k={k!r}: expected 0 <= k < {x.numel()}")
    res = torch.empty(3, dtype=torch.int32, device=x.device)
    _select(x, x.numel(), res, rank_host=int(k), largest=largest)
    return res[0:1].view(torch.float32)[0], res[1], res[2]


def _percentages(q, what="q"):
    q = [float(v) for v in (q if isinstance(q, (tuple, list)) else (q,))]
    if not 1 <= len(q) <= 4:
        raise ValueError(f"{what}: 1 to 4 percentages expected, got {len(q)}")
    if not all(0.0 <= v <= 100.0 for v in q):
        raise ValueError(f"{what}={q!r}: percentages in [0, 100] expected")
    return q


def percentile(x: torch.Tensor, q, channel_wise: bool = False) -> torch.Tensor:
    """``np.percentile(x, q)`` (linear rule) of a contiguous float32 device tensor, for 1 to 4 percentages in [0, 100]: with
    pos = q/100 * (n-1) and lo = floor(pos) the result is v[lo] + (v[lo+1] - v[lo]) * (pos - lo) in double, v[.] being exact order
    statistics (one select each; v[lo+1] only where pos is not an integer).  Returns float64 [len(q)] on the device, or [C, len(q)]
    with ``channel_wise=True`` (one row per index of dim 0).  Does not synchronise; no limit at 16 M elements."""
    _check_array(x)
    q = _percentages(q)
    rows = x.shape[0] if channel_wise else 1
    if channel_wise and x.dim() < 2:
        raise ValueError("channel_wise=True needs a tensor [C, ...]")
    n = x.numel() // rows
    flat = x.view(rows, n)
    ranks, fracs = [], []
    for v in q:
        pos = v / 100.0 * (n - 1)
        lo = min(int(math.floor(pos)), n - 1)
        ranks.append((lo, min(lo + 1, n - 1)))
        fracs.append(pos - lo)
    res = torch.zeros(rows, len(q), 2, 3, dtype=torch.int32, device=x.device)
    for r in range(rows):
        for j, (lo, hi) in enumerate(ranks):
            _select(flat[r], n, res[r, j, 0], rank_host=lo)
            if fracs[j] != 0.0:
                _select(flat[r], n, res[r, j, 1], rank_host=hi)
    v = res[..., 0].contiguous().view(torch.float32).double()           # [rows, len(q), 2]
    # the fractions are host numbers: scalar operands of the device arithmetic, no copy (no second statistic where one is 0)
    cols = []
    for j, f in enumerate(fracs):
        lo, hi = v[:, j, 0], v[:, j, 1]
        # numpy's own form of the interpolation: from the nearer end
        cols.append(lo if f == 0.0 else lo + (hi - lo) * f if f < 0.5 else hi - (hi - lo) * (1.0 - f))
    out = torch.stack(cols, dim=1)
    return out if channel_wise else out[0]


class TopKCEFn(torch.autograd.Function):
    """unetr_topkce_fwd / unetr_topkce_bwd.  The per-voxel values are an ordinary torch allocation saved for backward (backward
    compares their bits with the threshold); `k` is the one-element device tensor the kernels read."""

    @staticmethod
    def forward(ctx, logits, label, k, cfg, class_weight=None):
        logits, label, B, C, V = Fn._loss_inputs(logits, label, cfg["multilabel"])
        if class_weight is not None and class_weight.numel() != C:
            raise ValueError(f"class_weight has {class_weight.numel()} entries for {C} channels")
        d = TopKCEDesc(B=B, C=C, V=V, **cfg)
        d.class_weight = class_weight.data_ptr() if class_weight is not None else None
        values = torch.empty(B * V, dtype=torch.float32, device=logits.device)
        out = torch.empty(4, dtype=torch.float32, device=logits.device)
        coef = torch.empty(4, dtype=torch.float32, device=logits.device)
        ws = Fn.workspace(logits.device)
        call("unetr_topkce_fwd", ctypes.byref(d), logits.data_ptr(), label.data_ptr(), k.data_ptr(), values.data_ptr(), out.data_ptr(),
             coef.data_ptr(), ws.data_ptr(), ws.numel() * 4, Fn._stream())
        ctx.save_for_backward(logits, label, values, coef)
        ctx.desc, ctx.class_weight = d, class_weight            # (the tensor is kept alive with the pointer the descriptor holds)
        return out[0]

    @staticmethod
    def backward(ctx, dout):
        logits, label, values, coef = ctx.saved_tensors
        dloss = dout.reshape(1).contiguous()
        dlogits = torch.empty_like(logits)
        call("unetr_topkce_bwd", ctypes.byref(ctx.desc), logits.data_ptr(), label.data_ptr(), values.data_ptr(), coef.data_ptr(),
             dloss.data_ptr(), dlogits.data_ptr(), Fn._stream())
        return dlogits, None, None, None, None


def _check_k(k):
    k = float(k)
    if not 0.0 < k <= 100.0:
        raise ValueError(f"k={k!r}: a percentage in (0, 100] expected")
    return k


class TopKLoss(nn.Module):
    """Cross entropy averaged over the k % hardest voxels of the WHOLE batch (nnU-Net's TopKLoss): with u_v the per-voxel cross
    entropy (times ``class_weight[y_v]``), N the voxels that have one and K = max(1, floor(N * k / 100)), the mean of the K largest
    u -- ``torch.topk(u, K).values.mean()``.  Voxels that tie with the K-th value share its remaining weight equally in the gradient.
    Two input forms, as SegLoss has them:
      * ``to_onehot_y=True, softmax=True``: target [B,1,*spatial] class ids;
      * ``to_onehot_y=False, sigmoid=True``: target [B,C,*spatial] float mask, the class of a voxel is the first argmax of its mask.
    ``ignore_index`` and ``class_weight`` need class-id targets.  ``k`` lives in device memory (``.k``, one float32): ``set_k`` changes
    it without a synchronisation, also between the replays of a captured step."""

    def __init__(self, k: float = 10.0, to_onehot_y: bool = False, softmax: bool = False, sigmoid: bool = False, class_weight=None,
                 ignore_index=None, reduction: str = "mean") -> None:
        super().__init__()
        k = _check_k(k)
        lc.require_mean(reduction)
        multilabel = lc.activation_form(to_onehot_y, softmax, sigmoid)
        if ignore_index is not None and multilabel:
            raise NotImplementedError("ignore_index needs class-id targets (to_onehot_y=True)")
        if class_weight is not None:
            if multilabel:
                raise NotImplementedError("class_weight needs class-id targets (to_onehot_y=True)")
            class_weight = lc.class_weight_list(class_weight)
        self.class_weight = class_weight
        self.cfg = dict(multilabel=int(multilabel), has_ignore=int(ignore_index is not None),
                        ignore_index=int(ignore_index) if ignore_index is not None else 0)
        self._cw = {}      # device -> class_weight as a device buffer, created at first use
        self.register_buffer("k", lc.device_scalar(k), persistent=False)

    def set_k(self, k: float) -> None:
        """write the device scalar (a fill launch on the current stream, no synchronisation)"""
        self.k.fill_(_check_k(k))

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        lc.check_call(input, target, self.cfg, self.class_weight)
        k = lc.scalar_on(self, "k", input, "k")
        return TopKCEFn.apply(input, target, k, self.cfg, lc.weights_on(self._cw, self.class_weight, input.device))


class DiceTopKLoss(nn.Module):
    """nnU-Net's DC_and_topk_loss: ``lambda_dice * Dice + lambda_topk * TopK`` -- ``SegLoss(region="dice" or "jaccard",
    voxel="none")`` plus ``TopKLoss``; ``class_weight`` weighs the top-k term, ``ignore_index`` holds for both."""

    def __init__(self, k: float = 10.0, lambda_dice: float = 1.0, lambda_topk: float = 1.0, include_background: bool = True,
                 squared_pred: bool = False, jaccard: bool = False, batch: bool = False, smooth_nr: float = 1e-5,
                 smooth_dr: float = 1e-5, class_weight=None, ignore_index=None, to_onehot_y: bool = False, softmax: bool = False,
                 sigmoid: bool = False, other_act=None, reduction: str = "mean") -> None:
        super().__init__()
        act = _activation("DiceTopKLoss", to_onehot_y, softmax, sigmoid, other_act)
        self.topk = TopKLoss(k=k, class_weight=class_weight, ignore_index=ignore_index, reduction=reduction, **act)
        self.dice = SegLoss(region="jaccard" if jaccard else "dice", voxel="none", include_background=include_background,
                            squared_pred=squared_pred, batch=batch, smooth_nr=smooth_nr, smooth_dr=smooth_dr,
                            ignore_index=ignore_index, reduction=reduction, **act)
        self.lambda_dice, self.lambda_topk = float(lambda_dice), float(lambda_topk)

    def set_k(self, k: float) -> None:
        self.topk.set_k(k)

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return self.lambda_dice * self.dice(input, target) + self.lambda_topk * self.topk(input, target)
