"""Plain-torch float64 restatement of the top-k cross entropy (TopKLoss): the mean of the K largest per-voxel cross entropies of the
whole batch, with the symmetric tie rule written out.

  u_v = w[y_v] * -log softmax(z)[y_v]       (y_v: the label, or the first argmax of the mask; an ignored voxel has no value)
  N = voxels with a value,  K = max(1, floor(N * k / 100))  with k rounded to float32 first, as the device scalar holds it
  t = K-th largest u,  n_gt = #{u > t},  n_eq = #{u == t}
  weight of a voxel: 1/K where u > t, (K - n_gt) / (n_eq * K) where u == t, 0 elsewhere      (tie_weights; they sum to 1)
  X = sum_v weight_v * u_v = (sum_{u>t} u + (K - n_gt) t) / K

``topk_ref`` returns X as a float64 scalar that carries autograd back to ``logits``: the weights are constants of the gradient, so
dX/du_v is exactly the rule above.  Written from the formulas with a full sort -- no histogram, no shortcut the kernels take."""
import numpy as np
import torch
import torch.nn.functional as F


def k_count(N, k):
    """K of N valued voxels at percentage k (float32, as the device holds it), in double"""
    return max(1, min(int(np.floor(float(N) * float(np.float32(k)) / 100.0)), int(N)))


def voxel_values(logits, target, to_onehot_y=True, class_weight=None, ignore_index=None):
    """(u [B, V] float64 with autograd, valid [B, V] bool)"""
    z = logits.double()
    B, C = z.shape[0], z.shape[1]
    z = z.reshape(B, C, -1)
    logp = torch.log_softmax(z, 1)
    if to_onehot_y:
        lab = target.reshape(B, -1).long()
        valid = (lab != ignore_index) if ignore_index is not None else torch.ones_like(lab, dtype=torch.bool)
        cls = torch.where(valid, lab, torch.zeros_like(lab))
    else:
        if ignore_index is not None or class_weight is not None:
            raise NotImplementedError("class-id targets only")
        cls = torch.argmax(target.reshape(B, C, -1).double(), dim=1)      # first maximum
        valid = torch.ones_like(cls, dtype=torch.bool)
    u = -logp.gather(1, cls.unsqueeze(1))[:, 0]
    if class_weight is not None:
        u = u * torch.as_tensor(class_weight, dtype=torch.float64)[cls]
    return u, valid


def tie_weights(u, K):
    """weights [n] of the values u [n] (float64, all of them valued) under the symmetric tie rule"""
    s = torch.sort(u.detach(), descending=True).values
    t = s[K - 1]
    gt, eq = u.detach() > t, u.detach() == t
    n_gt, n_eq = int(gt.sum()), int(eq.sum())
    w = torch.zeros_like(u.detach())
    w[gt] = 1.0 / K
    w[eq] = (K - n_gt) / (n_eq * K)
    return w


def threshold_gap(u, K):
    """relative gap between the K-th and the (K+1)-th largest of u [n] (inf when there is no (K+1)-th)"""
    s = torch.sort(u.detach().double(), descending=True).values
    if K >= s.numel():
        return float("inf")
    return float((s[K - 1] - s[K]) / s[K - 1])


def topk_ref(logits, target, k=10.0, to_onehot_y=False, softmax=False, sigmoid=False, class_weight=None, ignore_index=None,
             per_item=False):
    """X of TopKLoss(k, ...).  per_item=True is NOT the loss: the mean over the batch items of each item's own top-k, what a
    per-item implementation would compute (the batch-scope test tells the two apart)."""
    u, valid = voxel_values(logits, target, to_onehot_y, class_weight, ignore_index)
    if per_item:
        return torch.stack([_topk_mean(u[b][valid[b]], k) for b in range(u.shape[0])]).mean()
    return _topk_mean(u[valid], k)


def _topk_mean(u, k):
    K = k_count(u.numel(), k)
    return (tie_weights(u, K) * u).sum()


def case_gap(logits, target, k, **kw):
    """the threshold gap of one (input, k) case, for the precondition the GPU cases are held to"""
    kw = {a: b for a, b in kw.items() if a in ("to_onehot_y", "class_weight", "ignore_index")}
    u, valid = voxel_values(logits, target, **kw)
    u = u[valid]
    return threshold_gap(u, k_count(u.numel(), k))


def eager_topk(logits, target, k):
    """the composition the loss replaces: cross_entropy(reduction="none") -> torch.topk -> mean (class-id targets, float64)"""
    B = logits.shape[0]
    ce = F.cross_entropy(logits.double(), target.reshape(B, *logits.shape[2:]).long(), reduction="none").reshape(-1)
    return torch.topk(ce, k_count(ce.numel(), k)).values.mean()
