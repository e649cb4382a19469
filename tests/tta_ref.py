"""CPU float64 reference for mirror test-time augmentation and ensembling in SlidingWindowInferer (a helper, not a test file).

The feature's definition is

    out[b, c, p] = sum_m sum_{windows k covering p} sum_{f in F} w(p - k) * unflip_f(act(net_m(flip_f(x_b[k : k + roi]))))[c, p - k]
    count[b, p]  = sum_m sum_k sum_f w(p - k);     result = out / count

``w`` does not depend on m or f, so with ``P(win) = mean over m, f of unflip_f(act(net_m(flip_f(win))))`` the result is
``sum_k w * P / sum_k w``: plain sliding-window blending of the predictor P.  ``tta_predictor`` builds P and
``ref_tta_sliding_window`` hands it to ``inference_ref.ref_sliding_window`` unchanged.
"""
import torch

from inference_ref import ref_sliding_window


def mask_dims(mask):
    """tensor dims of a [n, C, z, y, x] batch that flip mask `mask` (bit a = spatial axis a) reverses"""
    return [2 + a for a in range(3) if (mask >> a) & 1]


def flip(t, mask):
    dims = mask_dims(mask)
    return torch.flip(t, dims) if dims else t


def activate(t, activation):
    if activation == "softmax":
        return torch.softmax(t, dim=1)
    if activation == "sigmoid":
        return torch.sigmoid(t)
    assert activation is None
    return t


def tta_predictor(nets, masks, activation=None):
    def predict(win):
        acc = None
        for net in nets:
            for m in masks:
                seg = net(flip(win, m))
                if isinstance(seg, (tuple, list)):
                    seg = seg[-1]
                seg = flip(activate(seg.double(), activation), m)
                acc = seg if acc is None else acc + seg
        return acc / (len(nets) * len(masks))
    return predict


def ref_tta_sliding_window(inputs, roi, sw_batch_size, nets, masks, activation=None, overlap=0.25, importance=None, cval=0.0):
    """inputs: CPU tensor [B, Cin, D, H, W] (any float dtype; computed in float64); importance: [rz, ry, rx] or None (ones)"""
    imp = None if importance is None else importance.double()
    return ref_sliding_window(inputs.double(), roi, sw_batch_size, tta_predictor(nets, masks, activation), overlap=overlap,
                              importance=imp, cval=cval)
