"""Sliding-window inference and the Dice metric behind the reference's validation loop
(/root/reference/unetr_segmentation_3d.py:103-132), with MONAI 0.6.0's call signatures:

    val_outputs = sliding_window_inference(val_inputs, (crop, crop, crop), 4, model)           # :110
    dice_metric = DiceMetric(include_background=True, reduction="mean", get_not_nans=False)    # :485
    dice_metric(y_pred=[one-hot ...], y=[one-hot ...]); dice_metric.aggregate(); dice_metric.reset()   # :118-131

The window forward is the HIP hot path (run under torch.no_grad); blending and the Dice sums are the HIP kernels of
csrc/inference.hip.  Window geometry (scan interval, dense patch starts, padding of small volumes) is host integer logic
restated from MONAI 0.6.0 (monai/inferers/utils.py, monai/data/utils.py::dense_patch_slices).  No CPU fallback.

``SlidingWindowInferer`` (monai.inferers.SlidingWindowInferer's constructor + ``use_graph``, ``__call__(inputs, network,
post=None)``) is the same computation without per-window host work: the windows of a call are planned once into a device-resident
table (rows of ``sw_batch_size`` windows), and each row is advance -> gather -> forward -> accumulate over that table
(unetr_sw_gather_batch / unetr_sw_accumulate_batch: one launch each per row).  For this package's UNETR the row is captured
into one hipGraph per (model, precision, roi, batch size, input channels) and replayed for every row of every volume: volume
sizes live in a device-side descriptor, not in kernel arguments.  ``post`` fuses AsDiscrete / Activations into the finalize pass.
Both routes forward the same window batches in the same order and blend with the same fp32 operations as the per-window
function, so their results are bit-identical to it.

``mode="gaussian"``: MONAI is not installed where this was written, so the Gaussian importance map is RESTATED from memory of
MONAI 0.6.0 (monai/data/utils.py::compute_importance_map + monai/networks/layers/simplelayers.py::GaussianFilter /
convutils.gaussian_1d(approx="erf")) -- recalled, not pinned against the library; tests/inference_ref.py holds the same map
by real separable filtering.
"""
import math
import weakref
from typing import Callable, Sequence, Union

import torch
import torch.nn.functional as F

from . import _capi
from . import functional as Fn
from ._capi import call


def _scan_interval(image_size, roi_size, overlap):
    out = []
    for i, r in zip(image_size, roi_size):
        if r == i:
            out.append(int(r))
        else:
            interval = int(r * (1 - overlap))
            out.append(interval if interval > 0 else 1)
    return out


def _dense_patch_starts(image_size, patch_size, scan_interval):
    """window start corners in MONAI's order (meshgrid indexing='ij': last spatial dim fastest)"""
    starts = []
    for i, p, s in zip(image_size, patch_size, scan_interval):
        if s == 0:
            num = 1
        else:
            n = int(math.ceil(float(i) / s))
            first = next((d for d in range(n) if d * s + p >= i), None)
            num = first + 1 if first is not None else 1
        dim = []
        for idx in range(num):
            st = idx * s
            st -= max(st + p - i, 0)
            dim.append(st)
        starts.append(dim)
    return [(z, y, x) for z in starts[0] for y in starts[1] for x in starts[2]]


def _check_mode(mode):
    if mode not in ("constant", "gaussian"):
        raise ValueError(f"{mode!r} is not a valid BlendMode")          # what monai.utils.BlendMode(mode) raises


def _gaussian_1d(sigma):
    """monai.networks.layers.convutils.gaussian_1d(sigma, truncated=4.0, approx="erf", normalize=False), fp32"""
    tail = int(max(float(sigma) * 4.0, 0.5) + 0.5)
    x = torch.arange(-tail, tail + 1, dtype=torch.float32)
    t = 0.70710678 / abs(float(sigma))
    return (0.5 * ((t * (x + 0.5)).erf() - (t * (x - 0.5)).erf())).clamp(min=0), tail


def importance_map(roi_size, mode="constant", sigma_scale=0.125):
    """monai.data.utils.compute_importance_map (0.6.0) as a CPU fp32 tensor [rz, ry, rx].  "gaussian": a unit impulse at roi // 2
    filtered along z, y, x by the erf-approximated Gaussian of sigma = roi * sigma_scale (zero padding), divided by its maximum,
    clamped from below to its smallest non-zero entry.  Filtering an impulse with a separable kernel has a closed form -- the 1-D
    kernels read at offsets i - roi // 2 (zero beyond the tail), multiplied in filtering order (kz * ky) * kx -- which is what is
    evaluated here, with torch CPU fp32 ops."""
    _check_mode(mode)
    roi = [int(r) for r in roi_size]
    if mode == "constant":
        return torch.ones(roi, dtype=torch.float32)
    sig = list(sigma_scale) if isinstance(sigma_scale, (tuple, list)) else [sigma_scale] * len(roi)
    if len(sig) != len(roi):
        raise ValueError(f"sigma_scale: sequence must have length {len(roi)}, got {len(sig)}.")      # ensure_tuple_rep
    prof = []
    for r, sc in zip(roi, sig):
        k, tail = _gaussian_1d(r * sc)
        off = torch.arange(r) - r // 2
        inside = off.abs() <= tail
        prof.append(torch.where(inside, k[(off + tail).clamp(0, 2 * tail)], torch.zeros((), dtype=torch.float32)))
    m = (prof[0][:, None, None] * prof[1][None, :, None]) * prof[2][None, None, :]
    m = m / m.max()
    return m.clamp(min=m[m != 0].min())


_IMP = {}


def _device_importance_map(roi, mode, sigma_scale, device):
    """the importance map on `device` (computed on the host once per (roi, sigma_scale, device)); None for the constant mode"""
    _check_mode(mode)
    if mode == "constant":
        return None
    key = (tuple(roi), tuple(sigma_scale) if isinstance(sigma_scale, (tuple, list)) else float(sigma_scale), str(device))
    imp = _IMP.get(key)
    if imp is None:
        imp = _IMP[key] = importance_map(roi, mode, sigma_scale).to(device).contiguous()
    return imp


@torch.no_grad()
def sliding_window_inference(inputs: torch.Tensor, roi_size: Union[Sequence[int], int], sw_batch_size: int,
                             predictor: Callable[..., torch.Tensor], overlap: float = 0.25, mode: str = "constant",
                             sigma_scale: float = 0.125, padding_mode: str = "constant", cval: float = 0.0,
                             *args, **kwargs) -> torch.Tensor:
    Fn._require_gpu(inputs)
    if inputs.dim() != 5:
        raise ValueError("3-D volumes [B,C,D,H,W] expected")
    if overlap < 0 or overlap >= 1:
        raise AssertionError("overlap must be >= 0 and < 1.")
    _check_mode(mode)
    B = inputs.shape[0]
    image_size_ = list(inputs.shape[2:])
    roi = [roi_size] * 3 if isinstance(roi_size, int) else list(roi_size)
    roi = [r if r and r > 0 else i for r, i in zip(roi, image_size_)]           # fall_back_tuple
    image_size = [max(i, r) for i, r in zip(image_size_, roi)]
    pad = []
    for k in range(4, 1, -1):
        diff = max(roi[k - 2] - inputs.shape[k], 0)
        half = diff // 2
        pad.extend([half, diff - half])
    if any(pad):
        inputs = F.pad(inputs, pad=pad, mode=padding_mode, value=cval)
    inputs = inputs.contiguous()
    interval = _scan_interval(image_size, roi, overlap)
    starts = _dense_patch_starts(image_size, roi, interval)
    num_win = len(starts)
    total = num_win * B
    imp = _device_importance_map(roi, mode, sigma_scale, inputs.device)      # None: constant importance map (all ones)
    D, H, W = image_size
    V = D * H * W
    out = count = None
    stream = Fn._stream()
    for g0 in range(0, total, sw_batch_size):
        idxs = range(g0, min(g0 + sw_batch_size, total))
        wins = []
        for idx in idxs:
            b, (z, y, x) = idx // num_win, starts[idx % num_win]
            wins.append(inputs[b:b + 1, :, z:z + roi[0], y:y + roi[1], x:x + roi[2]])
        seg = predictor(torch.cat(wins), *args, **kwargs)
        if isinstance(seg, (tuple, list)):
            seg = seg[-1]                       # the reference UNETR returns (enc4, logits)
        seg = seg.contiguous().float()
        C = seg.shape[1]
        if out is None:
            out = torch.zeros(B, C, D, H, W, dtype=torch.float32, device=inputs.device)
            count = torch.zeros(B, D, H, W, dtype=torch.float32, device=inputs.device)
        for j, idx in enumerate(idxs):
            b, (z, y, x) = idx // num_win, starts[idx % num_win]
            call("unetr_sw_accumulate", seg[j].data_ptr(), imp.data_ptr() if imp is not None else None,
                 out[b].data_ptr(), count[b].data_ptr(), C, roi[0], roi[1], roi[2], D, H, W, z, y, x, stream)
    call("unetr_sw_finalize", out.data_ptr(), count.data_ptr(), B, out.shape[1], V, stream)
    sl = [slice(None), slice(None)]
    for sp in range(3):                       # undo the padding of volumes smaller than the window
        lo = pad[(2 - sp) * 2]
        sl.append(slice(lo, lo + image_size_[sp]))
    return out[tuple(sl)]


def dice_counts(pred: torch.Tensor, y: torch.Tensor, from_logits: bool) -> torch.Tensor:
    """[B, C, 3] float64 sums (pred*y, pred, y) from the HIP kernel"""
    Fn._require_gpu(pred)
    pred = pred.contiguous()
    y = y.contiguous().float()
    B, C = pred.shape[0], pred.shape[1]
    V = pred.numel() // (B * C)
    if from_logits and y.numel() != B * V:
        raise ValueError("from_logits: y must hold one class id per voxel [B,1,*spatial]")
    if not from_logits and y.shape != pred.shape:
        raise ValueError("y_pred and y must have the same one-hot shape")
    counts = torch.empty(B, C, 3, dtype=torch.float64, device=pred.device)
    ws = Fn.workspace(pred.device)
    call("unetr_dice_counts", pred.data_ptr(), y.data_ptr(), B, C, V, int(from_logits), counts.data_ptr(), ws.data_ptr(),
         ws.numel() * 4, Fn._stream())
    return counts


class DiceMetric:
    """monai.metrics.DiceMetric (0.6.0) for the reference's two instances: reduction "mean" and "mean_batch",
    include_background=True, get_not_nans=False.  ``__call__`` takes batched tensors or lists of per-item one-hot
    tensors (what decollate_batch + AsDiscrete produce at unetr_segmentation_3d.py:111-117) and buffers per-item
    per-class Dice (NaN where the ground truth class is absent); ``from_logits`` fuses argmax + one-hot (post_pred /
    post_label at :405-406) into the counting kernel."""

    def __init__(self, include_background: bool = True, reduction: str = "mean", get_not_nans: bool = False):
        if not include_background or get_not_nans or reduction not in ("mean", "mean_batch"):
            raise NotImplementedError("DiceMetric(include_background=True, reduction='mean'|'mean_batch', get_not_nans=False)")
        self.reduction = reduction
        self._buf = []

    @staticmethod
    def _stack(v):
        return torch.stack(list(v)) if isinstance(v, (list, tuple)) else v

    def __call__(self, y_pred, y, from_logits: bool = False):
        y_pred, y = self._stack(y_pred), self._stack(y)
        c = dice_counts(y_pred, y, from_logits)
        inter, po, yo = c[..., 0], c[..., 1], c[..., 2]
        f = torch.where(yo > 0, 2.0 * inter / (yo + po), torch.full_like(yo, float("nan"))).float()
        self._buf.append(f)
        return f

    def aggregate(self):
        f = torch.cat(self._buf).clone()
        nans = torch.isnan(f)
        not_nans = (~nans).float()
        f[nans] = 0
        zero = torch.zeros(1, device=f.device)
        if self.reduction == "mean":
            nn_c = not_nans.sum(dim=1)
            f = torch.where(nn_c > 0, f.sum(dim=1) / nn_c, zero)      # channel average
            nn_b = (nn_c > 0).float().sum(dim=0)
            return torch.where(nn_b > 0, f.sum(dim=0) / nn_b, zero)   # batch average
        nn_b = not_nans.sum(dim=0)
        return torch.where(nn_b > 0, f.sum(dim=0) / nn_b, zero)       # "mean_batch": per class

    def reset(self):
        self._buf = []


# ---- SlidingWindowInferer: table-driven rows, captured forward, fused post-processing ------------------------------------------
_POST = {None: 0, "onehot": 1, "argmax": 2, "sigmoid": 3}
_ACTIVATION = {None: 0, "softmax": 1, "sigmoid": 2}      # unetr_sw_volume.activation
_SOFTMAX_MAX_CHANNELS = 16


def flip_masks(tta_flips):
    """``tta_flips`` of SlidingWindowInferer as a list of flip masks (bit a = spatial axis a, the convention of
    augment.PARAM_COLS), or None: "all" is masks 0..7; otherwise a non-empty sequence without repeats of axis tuples or masks."""
    if tta_flips is None:
        return None
    if isinstance(tta_flips, str):
        if tta_flips != "all":
            raise ValueError(f"tta_flips must be None, 'all' or a sequence of axis tuples / masks, got {tta_flips!r}")
        return list(range(8))
    if not isinstance(tta_flips, (list, tuple)) or len(tta_flips) == 0:
        raise ValueError(f"tta_flips must be None, 'all' or a non-empty sequence of axis tuples / masks, got {tta_flips!r}")
    masks = []
    for f in tta_flips:
        if isinstance(f, bool):
            raise ValueError(f"tta_flips: {f!r} is neither an axis tuple nor a mask")
        if isinstance(f, int):
            if not 0 <= f <= 7:
                raise ValueError(f"tta_flips: mask {f} is outside 0..7")
            m = f
        elif isinstance(f, (list, tuple)):
            if any(isinstance(a, bool) or not isinstance(a, int) or not 0 <= a <= 2 for a in f) or len(set(f)) != len(f):
                raise ValueError(f"tta_flips: {f!r} is not a tuple of distinct spatial axes 0..2")
            m = sum(1 << a for a in f)
        else:
            raise ValueError(f"tta_flips: {f!r} is neither an axis tuple nor a mask")
        if m in masks:
            raise ValueError(f"tta_flips: flip {f!r} is listed twice")
        masks.append(m)
    return masks


def _finalize_threshold(post, activation):
    """the threshold of post="sigmoid" on the averaged result: logits at 0, sigmoid probabilities at 0.5"""
    if post == "sigmoid" and activation == "softmax":
        raise ValueError("post='sigmoid' thresholds one channel at a time: it cannot follow activation='softmax'")
    return 0.5 if activation == "sigmoid" else 0.0


def plan_window_table(batch, image_size, roi, overlap, n, flips=None):
    """The windows of one call as rows of ``n`` slots, in the order sliding_window_inference visits them (batch item major, then
    _dense_patch_starts).  Returns (int32 CPU tensor [rows, SW_ROW_INTS] in the layout of include/unetr_hip.h: [active, 0, 0, 0,
    (b, z, y, x) per slot], list of active counts per row); only the last row may hold fewer than ``n`` windows.
    ``flips`` (a list of flip masks): every row becomes ``len(flips)`` consecutive rows with the same slots, one per flip in
    order, the mask in header int 1; the counts are repeated with them."""
    if not 1 <= n <= _capi.SW_MAX_BATCH:
        raise ValueError(f"sw_batch_size must be in [1, {_capi.SW_MAX_BATCH}], got {n}")
    starts = _dense_patch_starts(image_size, roi, _scan_interval(image_size, roi, overlap))
    num_win = len(starts)
    total = num_win * batch
    rows = (total + n - 1) // n
    table = torch.zeros(rows, _capi.SW_ROW_INTS, dtype=torch.int32)
    flat = [(idx // num_win,) + tuple(starts[idx % num_win]) for idx in range(total)]
    counts = []
    for r in range(rows):
        slots = flat[r * n:(r + 1) * n]
        counts.append(len(slots))
        table[r, 0] = len(slots)
        table[r, 4:4 + 4 * len(slots)] = torch.tensor(slots, dtype=torch.int32).flatten()
    if flips is not None:
        nf = len(flips)
        table = table.repeat_interleave(nf, dim=0)
        table[:, 1] = torch.tensor(list(flips), dtype=torch.int32).repeat(rows)
        counts = [c for c in counts for _ in range(nf)]
    return table, counts


class _CapturedRow:
    __slots__ = ("graph", "static_in", "seg", "as_is", "derived", "signature", "model")


class SlidingWindowInferer:
    """monai.inferers.SlidingWindowInferer (0.6.0) plus ``use_graph`` and the ``post`` argument of ``__call__``:

        inferer = SlidingWindowInferer(roi_size, sw_batch_size, overlap, mode, sigma_scale, padding_mode, cval, use_graph=True)
        out = inferer(inputs, network, post=None)

    post=None: the blended logits [B, C, D, H, W] (what sliding_window_inference returns, bit for bit); "onehot":
    AsDiscrete(argmax=True, to_onehot=True, n_classes=C) of them; "argmax": the class ids as float [B, 1, D, H, W]; "sigmoid":
    Activations(sigmoid=True) + AsDiscrete(threshold_values=True), i.e. 1.0 where the logit is >= 0.  All three come out of the
    finalize kernel in the pass that divides by the weight sum.  ``network`` is any callable (a tuple result means its last
    element).  For this package's UNETR / UNETRLogits with use_graph=True, one row of windows -- advance the device cursor,
    gather, forward, accumulate -- is ONE hipGraph per (model, precision, roi, batch size, input channels), replayed for every row
    of every volume size; a call is then a table upload, a descriptor upload, ``rows`` replays and one finalize launch, with no
    host synchronisation.  A last row with fewer windows runs through a second graph of exactly that batch size, so every route
    forwards the batch compositions the function forwards.  Anything else runs the same kernels eagerly.
    ``stats``: captures / recaptures / replays / eager_rows, counted over the inferer's life.

    Mirror test-time augmentation and ensembling (this project's semantics, per window as nnU-Net does):
    ``tta_flips`` -- None, "all" (flip masks 0..7) or a sequence of axis tuples ``()``, ``(0,)``, ``(1, 2)`` / masks 0..7 -- makes
    every window be forwarded once per flip, mirrored inside the gather, and blended un-mirrored inside the accumulate;
    ``activation`` -- None, "softmax" (at most 16 channels) or "sigmoid" -- is applied to each window prediction before it is
    blended; ``network`` may be a list or tuple of networks whose predictions are blended into the same sums, model after model:

        out[b, c, p] = sum_m sum_{windows k covering p} sum_{f in flips} w(p - k) * unflip_f(act(net_m(flip_f(x_b[k : k + roi]))))[c, p - k]
        count[b, p]  = the same sum of w(p - k);   result = out / count

    The weight w follows the position in the volume.  ``post`` works on that average: "sigmoid" thresholds at 0.5 after
    activation="sigmoid" and is an error after "softmax".  The rows of a call are the plan's rows times the flips (the flip mask is
    data in the row header), so the same captured graphs serve every flip; an ensemble takes the captured route when every member
    is this package's UNETR, and ``replays`` / ``eager_rows`` count rows x flips x models.

    Weight freshness of a captured forward: see derived_weights.invalidate_weight_shadows (rule for captured inference graphs)."""

    def __init__(self, roi_size, sw_batch_size: int = 1, overlap: float = 0.25, mode: str = "constant", sigma_scale=0.125,
                 padding_mode: str = "constant", cval: float = 0.0, use_graph: bool = True, tta_flips=None, activation=None):
        _check_mode(mode)
        if activation not in _ACTIVATION:
            raise ValueError(f"activation must be one of {list(_ACTIVATION)}, got {activation!r}")
        self.tta_flips = flip_masks(tta_flips)
        self.activation = activation
        if overlap < 0 or overlap >= 1:
            raise AssertionError("overlap must be >= 0 and < 1.")
        if not 1 <= int(sw_batch_size) <= _capi.SW_MAX_BATCH:
            raise ValueError(f"sw_batch_size must be in [1, {_capi.SW_MAX_BATCH}], got {sw_batch_size}")
        self.roi_size = roi_size
        self.sw_batch_size = int(sw_batch_size)
        self.overlap, self.mode, self.sigma_scale = overlap, mode, sigma_scale
        self.padding_mode, self.cval = padding_mode, float(cval)
        self.use_graph = bool(use_graph)
        self.stats = dict(captures=0, recaptures=0, replays=0, eager_rows=0)
        self._desc = {}        # device index -> uint8 tensor holding the unetr_sw_volume every launch of this inferer reads
        self._graphs = {}      # (id(model), precision, roi, batch size, Cin, device index) -> _CapturedRow
        self._inputs = {}      # eager route: (batch size, Cin, roi, device index) -> forward input buffer
        self._plans = {}
        self._keep = None      # table / staging of the call in flight

    # ------------------------------------------------------------------------------------------------ host side
    def _plan(self, B, image_size, roi):
        key = (B, tuple(image_size), tuple(roi))
        plan = self._plans.get(key)
        if plan is None:
            if len(self._plans) > 64:
                self._plans.clear()
            plan = self._plans[key] = plan_window_table(B, image_size, roi, self.overlap, self.sw_batch_size, self.tta_flips)
        return plan

    def _desc_of(self, device):
        d = self._desc.get(device.index)
        if d is None:
            import ctypes
            d = self._desc[device.index] = torch.zeros(ctypes.sizeof(_capi.SwVolume), dtype=torch.uint8, device=device)
        return d

    def _upload_desc(self, desc, vol):
        host = torch.frombuffer(bytearray(bytes(vol)), dtype=torch.uint8).pin_memory()
        desc.copy_(host, non_blocking=True)          # (the pinned block is not reused before the copy has run: caching host allocator)

    # ------------------------------------------------------------------------------------------------ one row
    @staticmethod
    def _gather(desc, static_in, roi):
        s = Fn._stream()
        call("unetr_sw_advance", desc.data_ptr(), s)
        call("unetr_sw_gather_batch", desc.data_ptr(), static_in.data_ptr(), static_in.shape[0], static_in.shape[1], *roi, s)

    @staticmethod
    def _forward(network, static_in, args, kwargs):
        seg = network(static_in, *args, **kwargs)
        if isinstance(seg, (tuple, list)):
            seg = seg[-1]
        seg = seg.contiguous().float()
        if seg.dim() != 5 or seg.shape[0] != static_in.shape[0] or tuple(seg.shape[2:]) != tuple(static_in.shape[2:]):
            raise ValueError(f"network returned {tuple(seg.shape)} for windows {tuple(static_in.shape)}")
        return seg

    @staticmethod
    def _accumulate(desc, seg, imp, roi):
        call("unetr_sw_accumulate_batch", desc.data_ptr(), seg.data_ptr(), imp.data_ptr() if imp is not None else None,
             seg.shape[0], seg.shape[1], *roi, Fn._stream())

    # ------------------------------------------------------------------------------------------------ capture
    @staticmethod
    def _derived_entries(model):
        """the record of every derived weight copy a forward reads that is registered for the model's parameters"""
        return Fn.records_of(model.parameters())

    @staticmethod
    def _signature(model, device, derived):
        """every address a captured forward may have baked in: the parameters, the scratch workspace, and the buffers of the
        derived copies that existed when it was captured (`derived`: their records then, looked up again)"""
        sig = [p.data_ptr() for p in model.parameters()]
        sig.append(Fn.workspace(device).data_ptr())
        for rec in derived:
            cur = rec.current()
            sig.append(cur.buf.data_ptr() if cur is not None else 0)
        return tuple(sig)

    @classmethod
    def _as_is(cls, model):
        """the derived copies a capture starting now would READ AS THEY ARE (optimizer-maintained, or the word shadow in step with
        its parameter) instead of re-deriving them inside the graph"""
        return [rec for rec in cls._derived_entries(model) if rec.read_as_is()]

    def _capture(self, model, key, m, Cin, roi, desc, imp):
        from .train_step import side_stream
        device = desc.device
        cur = torch.cuda.current_stream(device)
        side = side_stream(device)
        ent = _CapturedRow()
        ent.model = weakref.ref(model)
        ent.static_in = torch.zeros(m, Cin, *roi, dtype=torch.float32, device=device)
        side.wait_stream(cur)
        with torch.cuda.stream(side), torch.no_grad():
            Fn.workspace(device)                       # exists before capture, outside the graph's private pool
            self._forward(model, ent.static_in, (), {})  # eager warm-up: derived weight copies and buffers come to exist
        cur.wait_stream(side)
        torch.cuda.synchronize(device)
        ent.as_is = self._as_is(model)
        ent.graph = torch.cuda.CUDAGraph()
        # (thread-local capture mode: a live process group's watchdog thread polls events, see TrainStep._capture)
        with torch.cuda.graph(ent.graph, stream=side, capture_error_mode="thread_local"), torch.no_grad():
            self._gather(desc, ent.static_in, roi)
            ent.seg = self._forward(model, ent.static_in, (), {})
            self._accumulate(desc, ent.seg, imp, roi)
        cur.wait_stream(side)
        ent.derived = self._derived_entries(model)
        ent.signature = self._signature(model, device, ent.derived)
        self._graphs[key] = ent
        self.stats["captures"] += 1
        return ent

    def _refresh(self, model, ents):
        """Before the first replay of a call: the copies the graphs read as they are go through their getters eagerly in a new
        weight epoch -- nothing happens to a copy that is still optimizer-maintained and in step; a stale one is re-derived into
        the buffer the graph reads.  False when an address a graph baked in has moved (the caller captures again)."""
        Fn.begin_forward(None)
        seen = set()
        for ent in ents:
            for rec in ent.as_is:
                p = rec.param()
                if p is None:
                    return False
                slot = (rec.kind, id(p), rec.pack)
                if slot not in seen:
                    seen.add(slot)
                    rec.get()
        device = ents[0].static_in.device
        return all(ent.signature == self._signature(model, device, ent.derived) for ent in ents)

    def _rows_captured(self, model, sizes, Cin, roi, desc, imp):
        """the graphs for the batch sizes of this call, captured or re-captured as needed, fresh for replay"""
        keys = {m: (id(model), model.precision, tuple(roi), m, Cin, desc.device.index, None if imp is None else imp.data_ptr())
                for m in sizes}
        for m, key in keys.items():
            ent = self._graphs.get(key)
            if ent is not None and ent.model() is not model:
                del self._graphs[key]
                ent = None
            if ent is None:
                self._capture(model, key, m, Cin, roi, desc, imp)
        if not self._refresh(model, [self._graphs[k] for k in keys.values()]):
            for m, key in keys.items():
                del self._graphs[key]
                self._capture(model, key, m, Cin, roi, desc, imp)
                self.stats["recaptures"] += 1
            if not self._refresh(model, [self._graphs[k] for k in keys.values()]):
                raise RuntimeError("SlidingWindowInferer: weight buffers moved again right after a re-capture")
        return {m: self._graphs[k] for m, k in keys.items()}

    # ------------------------------------------------------------------------------------------------ call
    def _check_channels(self, C):
        if self.activation == "softmax" and C > _SOFTMAX_MAX_CHANNELS:
            raise NotImplementedError(f"activation='softmax' takes at most {_SOFTMAX_MAX_CHANNELS} channels, got {C}")

    @torch.no_grad()
    def __call__(self, inputs: torch.Tensor, network, post=None, *args, **kwargs) -> torch.Tensor:
        from .unetr import UNETR
        if post not in _POST:
            raise ValueError(f"post must be one of {list(_POST)}, got {post!r}")
        threshold = _finalize_threshold(post, self.activation)
        networks = list(network) if isinstance(network, (list, tuple)) else [network]
        if not networks:
            raise ValueError("network: an ensemble needs at least one member")
        Fn._require_gpu(inputs)
        if inputs.dim() != 5:
            raise ValueError("3-D volumes [B,C,D,H,W] expected")
        device = inputs.device
        B, Cin = inputs.shape[0], inputs.shape[1]
        image_size_ = list(inputs.shape[2:])
        roi_size = self.roi_size
        roi = [roi_size] * 3 if isinstance(roi_size, int) else list(roi_size)
        roi = [int(r) if r and r > 0 else i for r, i in zip(roi, image_size_)]           # fall_back_tuple
        image_size = [max(i, r) for i, r in zip(image_size_, roi)]
        pad = []
        for k in range(4, 1, -1):
            diff = max(roi[k - 2] - inputs.shape[k], 0)
            half = diff // 2
            pad.extend([half, diff - half])
        if any(pad) and self.padding_mode != "constant":
            inputs = F.pad(inputs, pad=pad, mode=self.padding_mode)       # the gather then reads a volume that needs no padding
            in_size, offs = image_size, (0, 0, 0)
        else:
            in_size, offs = image_size_, (pad[4], pad[2], pad[0])         # constant padding happens inside the gather
        inputs = inputs.contiguous().float()
        table_cpu, counts = self._plan(B, image_size, roi)
        n = self.sw_batch_size
        imp = _device_importance_map(roi, self.mode, self.sigma_scale, device)
        desc = self._desc_of(device)
        D, H, W = image_size
        V = D * H * W
        captured = self.use_graph and all(isinstance(net, UNETR) for net in networks) and not args and not kwargs
        known = {net.out_channels for net in networks if isinstance(net, UNETR)}
        if len(known) > 1:
            raise ValueError(f"the networks of an ensemble must return the same channel count, got {sorted(known)}")
        C = known.pop() if known else None
        if C is not None:
            self._check_channels(C)
        graphs = None
        if captured:
            # (every member's graphs exist, and are fresh, before the first replay: a capture synchronises the device)
            graphs = [self._rows_captured(net, sorted(set(counts)), Cin, roi, desc, imp) for net in networks]
        table = table_cpu.pin_memory().to(device, non_blocking=True)
        vol = _capi.SwVolume()
        vol.in_, vol.table = inputs.data_ptr(), table.data_ptr()
        vol.B, vol.Cin = B, Cin
        vol.Di, vol.Hi, vol.Wi = in_size
        vol.D, vol.H, vol.W = D, H, W
        vol.pz, vol.py, vol.px = offs
        vol.cval, vol.rows, vol.cursor = self.cval, len(counts), -1
        vol.activation = _ACTIVATION[self.activation]
        out = count = None

        def allocate(C):
            nonlocal out, count
            out = torch.zeros(B, C, D, H, W, dtype=torch.float32, device=device)
            count = torch.zeros(B, D, H, W, dtype=torch.float32, device=device)
            vol.out, vol.count, vol.C = out.data_ptr(), count.data_ptr(), C
            self._upload_desc(desc, vol)

        if C is not None:
            allocate(C)
        else:
            vol.out = vol.count = None
            vol.C = 0
            self._upload_desc(desc, vol)
        self._keep = (table, inputs)
        # models in list order, each over the whole table from row 0; out / count persist, the cursor is rewound in between
        for k, net in enumerate(networks):
            if k:
                call("unetr_sw_rewind", desc.data_ptr(), Fn._stream())
            if captured:
                for m in counts:
                    graphs[k][m].graph.replay()
                self.stats["replays"] += len(counts)
                continue
            for r, m in enumerate(counts):
                key = (m, Cin, tuple(roi), device.index)
                static_in = self._inputs.get(key)
                if static_in is None:
                    static_in = self._inputs[key] = torch.empty(m, Cin, *roi, dtype=torch.float32, device=device)
                self._gather(desc, static_in, roi)
                seg = self._forward(net, static_in, args, kwargs)
                if out is None:
                    self._check_channels(seg.shape[1])
                    vol.cursor = r                    # (the cursor has been advanced to this row already)
                    allocate(seg.shape[1])
                elif seg.shape[1] != out.shape[1]:
                    raise ValueError(f"network returned {seg.shape[1]} channels, {out.shape[1]} expected")
                self._accumulate(desc, seg, imp, roi)
            self.stats["eager_rows"] += len(counts)
        C = out.shape[1]
        dst = torch.empty(B, 1, D, H, W, dtype=torch.float32, device=device) if post == "argmax" else None
        call("unetr_sw_finalize_post_thr", out.data_ptr(), count.data_ptr(), dst.data_ptr() if dst is not None else None, B, C, V,
             _POST[post], threshold, Fn._stream())
        res = dst if dst is not None else out
        sl = [slice(None), slice(None)]
        for sp in range(3):                       # undo the padding of volumes smaller than the window
            lo = pad[(2 - sp) * 2]
            sl.append(slice(lo, lo + image_size_[sp]))
        return res[tuple(sl)]
