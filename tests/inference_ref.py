"""CPU restatement of MONAI 0.6.0 sliding-window blending with an importance map, for tests (a helper, not a test file).

MONAI is not installed where this was written: like oracle/unetr_oracle.py and tests/metrics_ref.py this is RESTATED from memory
of monai/data/utils.py::compute_importance_map, monai/networks/layers/simplelayers.py::GaussianFilter,
monai/networks/layers/convutils.py::gaussian_1d(approx="erf") and monai/inferers/utils.py::sliding_window_inference --
recalled, not pinned against the library.

* ``ref_importance_map``: the Gaussian map by REAL separable filtering of a unit impulse through F.conv3d (the package
  evaluates the closed form of that filtering).
* ``ref_sliding_window``: the per-window loop with an importance map.  Its window order and grouping are not restated: they are
  read off ``oracle_sliding_window_inference`` (imported, not edited) by sending a volume of voxel indices through it.
"""
import torch
import torch.nn.functional as F

from oracle.unetr_oracle import oracle_sliding_window_inference


def _gaussian_1d(sigma):
    tail = int(max(float(sigma) * 4.0, 0.5) + 0.5)
    x = torch.arange(-tail, tail + 1, dtype=torch.float32)
    t = 0.70710678 / abs(float(sigma))
    return (0.5 * ((t * (x + 0.5)).erf() - (t * (x - 0.5)).erf())).clamp(min=0)


def ref_importance_map(roi, mode="gaussian", sigma_scale=0.125):
    roi = [int(r) for r in roi]
    if mode == "constant":
        return torch.ones(roi, dtype=torch.float32)
    sig = list(sigma_scale) if isinstance(sigma_scale, (tuple, list)) else [sigma_scale] * 3
    m = torch.zeros(roi, dtype=torch.float32)
    m[roi[0] // 2, roi[1] // 2, roi[2] // 2] = 1.0
    m = m[None, None]
    for d in range(3):                                   # GaussianFilter: one 1-D convolution per axis, zero padding = tail
        k = _gaussian_1d(roi[d] * sig[d])
        shape, padding = [1, 1, 1, 1, 1], [0, 0, 0]
        shape[2 + d], padding[d] = k.numel(), k.numel() // 2
        m = F.conv3d(m, k.reshape(shape), padding=padding)
    m = m[0, 0]
    m = m / m.max()
    return m.clamp(min=m[m != 0].min())


def oracle_window_order(batch, image_size, roi, sw_batch_size, overlap):
    """groups of (b, z, y, x) window corners exactly as oracle_sliding_window_inference forwards them (image_size >= roi)"""
    D, H, W = image_size
    V = D * H * W
    idx = torch.arange(batch * V, dtype=torch.float64).reshape(batch, 1, D, H, W)
    groups = []

    def record(win):
        grp = []
        for v in win[:, 0, 0, 0, 0].tolist():
            v = int(v)
            b, r = divmod(v, V)
            z, r = divmod(r, H * W)
            y, x = divmod(r, W)
            grp.append((b, z, y, x))
        groups.append(grp)
        return torch.zeros(win.shape[0], 1, *win.shape[2:], dtype=win.dtype)

    oracle_sliding_window_inference(idx, tuple(roi), sw_batch_size, record, overlap=overlap)
    return groups


def ref_sliding_window(inputs, roi, sw_batch_size, predictor, overlap=0.25, importance=None, padding_mode="constant", cval=0.0):
    """sliding_window_inference on the CPU with importance map `importance` ([rz, ry, rx]; None = ones)"""
    roi = list(roi)
    size_ = list(inputs.shape[2:])
    pad = []
    for k in range(4, 1, -1):
        diff = max(roi[k - 2] - inputs.shape[k], 0)
        pad.extend([diff // 2, diff - diff // 2])
    if any(pad):
        inputs = F.pad(inputs, pad, mode=padding_mode, value=cval) if padding_mode == "constant" else F.pad(inputs, pad, mode=padding_mode)
    size = list(inputs.shape[2:])
    B = inputs.shape[0]
    imp = torch.ones(roi, dtype=inputs.dtype) if importance is None else importance.to(inputs.dtype)
    out = count = None
    for grp in oracle_window_order(B, size, roi, sw_batch_size, overlap):
        wins = torch.cat([inputs[b:b + 1, :, z:z + roi[0], y:y + roi[1], x:x + roi[2]] for b, z, y, x in grp])
        seg = predictor(wins)
        if out is None:
            out = torch.zeros(B, seg.shape[1], *size, dtype=seg.dtype)
            count = torch.zeros(B, seg.shape[1], *size, dtype=seg.dtype)
        for k, (b, z, y, x) in enumerate(grp):
            out[b, :, z:z + roi[0], y:y + roi[1], x:x + roi[2]] += imp * seg[k]
            count[b, :, z:z + roi[0], y:y + roi[1], x:x + roi[2]] += imp
    out = out / count
    return out[:, :, pad[4]:pad[4] + size_[0], pad[2]:pad[2] + size_[1], pad[0]:pad[0] + size_[2]]
