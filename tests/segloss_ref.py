"""Plain-torch float64 restatement of the segmentation loss family (SegLoss): loss = lambda_region * R + lambda_voxel * X.

``segloss_ref(logits, target, ...)`` takes SegLoss's arguments and returns (R, X) as float64 scalars that carry autograd back to
``logits`` (cast to float64 on entry).  One-hot mode (to_onehot_y=True): target [B,1,*spatial] class ids, p = softmax(logits, 1).
Multilabel mode: target [B,C,*spatial] float mask, p = sigmoid(logits).  Written from the formulas, with no shortcut the kernel
takes: the probabilities and the one-hot target are materialised, the sums are torch sums, the gradient is autograd's."""
import torch
import torch.nn.functional as F


def _gdl_weights(G, w_type):
    """[N, C] weights from the target sums: 1/G^2, 1/G or 1; a channel with G = 0 takes the largest finite weight of its row, or 0"""
    if w_type == "square":
        w = 1.0 / (G * G)
    elif w_type == "simple":
        w = 1.0 / G
    elif w_type == "uniform":
        w = torch.ones_like(G)
    else:
        raise ValueError(w_type)
    w = w.detach().clone()                                  # constant for the gradient
    for row in w:
        finite = torch.isfinite(row)
        row[~finite] = row[finite].max() if finite.any() else 0.0
    return w


def segloss_ref(logits, target, region="dice", voxel="ce", include_background=True, to_onehot_y=False, softmax=False, sigmoid=False,
                squared_pred=False, batch=False, smooth_nr=1e-5, smooth_dr=1e-5, alpha=0.5, beta=0.5, w_type="square", gamma=2.0,
                class_weight=None, ignore_index=None, lambda_region=1.0, lambda_voxel=1.0):
    z = logits.double()
    B, C = z.shape[0], z.shape[1]
    z = z.reshape(B, C, -1)
    if to_onehot_y:
        lab = target.reshape(B, -1).long()
        valid = (lab != ignore_index) if ignore_index is not None else torch.ones_like(lab, dtype=torch.bool)
        y = F.one_hot(torch.where(valid, lab, torch.zeros_like(lab)), C).movedim(-1, 1).double()
        p = torch.softmax(z, 1)
    else:
        if ignore_index is not None:
            raise NotImplementedError("ignore_index")
        lab = None
        valid = torch.ones(B, z.shape[2], dtype=torch.bool)
        y = target.reshape(B, C, -1).double()
        p = torch.sigmoid(z)
    m = valid.unsqueeze(1).double()                          # an ignored voxel contributes to no sum at all
    if not include_background and C == 1:
        raise ValueError("include_background")
    c0 = 0 if include_background else 1
    cw = torch.as_tensor(class_weight, dtype=torch.float64) if class_weight is not None else None

    R = z.new_zeros(())
    if region != "none":
        if squared_pred and region in ("tversky", "generalized_dice"):
            raise NotImplementedError("squared_pred")
        I = (p * y * m).sum(2)[:, c0:]
        P = ((p * p if squared_pred else p) * m).sum(2)[:, c0:]
        G = ((y * y if squared_pred else y) * m).sum(2)[:, c0:]
        if batch:
            I, P, G = I.sum(0, keepdim=True), P.sum(0, keepdim=True), G.sum(0, keepdim=True)
        if region == "dice":
            f = 1.0 - (2.0 * I + smooth_nr) / (G + P + smooth_dr)
        elif region == "jaccard":
            f = 1.0 - (2.0 * I + smooth_nr) / (2.0 * (G + P - I) + smooth_dr)
        elif region == "tversky":
            f = 1.0 - (I + smooth_nr) / (I + alpha * (P - I) + beta * (G - I) + smooth_dr)
        elif region == "generalized_dice":
            w = _gdl_weights(G, w_type)
            f = 1.0 - (2.0 * (w * I).sum(1) + smooth_nr) / ((w * (G + P)).sum(1) + smooth_dr)
        else:
            raise ValueError(region)
        R = f.mean()

    X = z.new_zeros(())
    if voxel == "ce":
        logp = torch.log_softmax(z, 1)
        if to_onehot_y:
            w = cw if cw is not None else torch.ones(C, dtype=torch.float64)
            wv = (w[None, :, None] * y).sum(1) * m[:, 0]                # w_{y_v}, 0 where ignored
            X = (wv * -(logp * y).sum(1)).sum() / wv.sum()
        else:
            if cw is not None:
                raise NotImplementedError("class_weight")
            cls = torch.argmax(y, dim=1)                                # first maximum
            X = -logp.gather(1, cls.unsqueeze(1)).mean()
    elif voxel == "focal":
        bce = z.clamp_min(0) - z * y + torch.log1p(torch.exp(-z.abs()))
        val = torch.exp(gamma * F.logsigmoid(-z * (2.0 * y - 1.0))) * bce
        if cw is not None:
            val = val * cw[None, :, None]
        val = (val * m)[:, c0:]
        X = val.sum() / (m.sum() * (C - c0))
    elif voxel != "none":
        raise ValueError(voxel)
    return R, X
