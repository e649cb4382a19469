"""CPU tests of the segmentation loss family: the float64 reference (tests/segloss_ref.py) against the existing oracle and against
torch's own losses where the family contains them, the constructor's refusals, and the C ABI additions."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from segloss_ref import segloss_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONEHOT = dict(to_onehot_y=True, softmax=True)
MULTI = dict(to_onehot_y=False, sigmoid=True)


def _inputs(B, C, S, seed=0, multilabel=False):
    gen = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, C, S, S, S, generator=gen, dtype=torch.float64) * 2
    if multilabel:
        return logits, (torch.rand(B, C, S, S, S, generator=gen) < 0.35).double()
    return logits, torch.randint(0, C, (B, 1, S, S, S), generator=gen).double()


def test_defaults_equal_the_dicece_oracle(pkg):
    """region="dice", voxel="ce" with the default smoothing is the DiceCELoss the oracle states, in both modes"""
    from oracle.unetr_oracle import oracle_dice_ce_terms
    assert pkg.SegLoss(**ONEHOT).region == "dice" and pkg.SegLoss(**ONEHOT).voxel == "ce"      # the defaults under test
    logits, label = _inputs(2, 3, 7, seed=1)
    d, c = oracle_dice_ce_terms(logits, label)
    R, X = segloss_ref(logits, label, **ONEHOT)
    assert abs(float(R - d)) < 1e-12 and abs(float(X - c)) < 1e-12
    logits, mask = _inputs(2, 4, 6, seed=2, multilabel=True)
    d, c = oracle_dice_ce_terms(logits, mask, to_onehot_y=False, softmax=False, sigmoid=True)
    R, X = segloss_ref(logits, mask, **MULTI)
    assert abs(float(R - d)) < 1e-12 and abs(float(X - c)) < 1e-12


def test_focal_gamma_zero_is_bce_with_logits(pkg):
    pkg.FocalLoss(gamma=0.0)
    logits, mask = _inputs(2, 3, 6, seed=3, multilabel=True)
    _, X = segloss_ref(logits, mask, region="none", voxel="focal", gamma=0.0)
    assert abs(float(X - F.binary_cross_entropy_with_logits(logits, mask))) < 1e-12
    logits, label = _inputs(2, 3, 6, seed=4)
    onehot = F.one_hot(label[:, 0].long(), 3).movedim(-1, 1).double()
    _, X = segloss_ref(logits, label, region="none", voxel="focal", gamma=0.0, to_onehot_y=True)
    assert abs(float(X - F.binary_cross_entropy_with_logits(logits, onehot))) < 1e-12


def test_weighted_ce_with_ignore_index_is_torch_cross_entropy(pkg):
    w = [0.2, 1.0, 3.0, 0.5]
    pkg.SegLoss(class_weight=w, ignore_index=255, **ONEHOT)
    logits, label = _inputs(2, 4, 6, seed=5)
    label[torch.rand(label.shape, generator=torch.Generator().manual_seed(6)) < 0.3] = 255
    _, X = segloss_ref(logits, label, class_weight=w, ignore_index=255, **ONEHOT)
    want = F.cross_entropy(logits, label[:, 0].long(), weight=torch.tensor(w, dtype=torch.float64), ignore_index=255)
    assert abs(float(X - want)) < 1e-12


def test_tversky_half_half_is_dice(pkg):
    """alpha = beta = 0.5: 1 - (I + nr) / (0.5 (P + G) + dr) = 1 - (2I + 2nr) / (G + P + 2dr)"""
    pkg.TverskyLoss(alpha=0.5, beta=0.5, **ONEHOT)
    for kw, multilabel in ((ONEHOT, False), (MULTI, True)):
        logits, t = _inputs(2, 3, 6, seed=7, multilabel=multilabel)
        Rt, _ = segloss_ref(logits, t, region="tversky", voxel="none", alpha=0.5, beta=0.5, smooth_nr=1e-3, smooth_dr=2e-3, **kw)
        Rd, _ = segloss_ref(logits, t, region="dice", voxel="none", smooth_nr=2e-3, smooth_dr=4e-3, **kw)
        assert abs(float(Rt - Rd)) < 1e-12


def test_generalized_dice_weight_of_an_absent_class(pkg):
    from segloss_ref import _gdl_weights
    pkg.GeneralizedDiceLoss(**ONEHOT)
    G = torch.tensor([[100.0, 0.0, 4.0], [50.0, 25.0, 10.0]], dtype=torch.float64)
    w = _gdl_weights(G, "square")
    assert w[0, 1] == w[0, 2] == 1.0 / 16.0 and w[1, 1] == 1.0 / 625.0      # the largest finite weight of THAT item
    w = _gdl_weights(G, "simple")
    assert w[0, 1] == 0.25
    # the same through the loss: class 1 absent from item 0
    logits, label = _inputs(2, 3, 6, seed=8)
    label[0][label[0] == 1] = 2
    z = logits.clone().requires_grad_(True)
    R, _ = segloss_ref(z, label, region="generalized_dice", voxel="none", **ONEHOT)
    R.backward()
    assert torch.isfinite(R) and torch.isfinite(z.grad).all() and 0.0 < float(R.detach()) < 1.0
    # every class absent from item 0 (an all-zero mask): no finite weight there, so all of them are 0 and f_0 = 1 - nr/dr
    w = _gdl_weights(torch.tensor([[0.0, 0.0], [3.0, 0.0]], dtype=torch.float64), "square")
    assert torch.isfinite(w).all() and w[0].tolist() == [0.0, 0.0] and w[1, 1] == 1.0 / 9.0
    logits, mask = _inputs(2, 3, 6, seed=9, multilabel=True)
    mask[0] = 0
    z = logits.clone().requires_grad_(True)
    R, _ = segloss_ref(z, mask, region="generalized_dice", voxel="none", **MULTI)
    R.backward()
    assert torch.isfinite(R) and torch.isfinite(z.grad).all()
    assert not z.grad[0].any()                                              # zero weights: item 0 has no gradient


def test_constructor_refusals(pkg):
    S = pkg.SegLoss
    for kw in (dict(), dict(to_onehot_y=True, sigmoid=True), dict(to_onehot_y=False, softmax=True), dict(reduction="sum", **ONEHOT),
               dict(region="tversky", squared_pred=True, **ONEHOT), dict(region="generalized_dice", squared_pred=True, **ONEHOT),
               dict(ignore_index=255, **MULTI), dict(class_weight=[1.0, 2.0], **MULTI)):
        with pytest.raises(NotImplementedError):
            S(**kw)
    with pytest.raises(NotImplementedError, match="squared_pred"):
        S(region="tversky", squared_pred=True, **ONEHOT)
    with pytest.raises(NotImplementedError, match="ignore_index"):
        S(ignore_index=0, **MULTI)
    with pytest.raises(NotImplementedError, match="class_weight"):
        S(class_weight=[1.0, 2.0], **MULTI)
    with pytest.raises(NotImplementedError, match="reduction"):
        pkg.DiceLoss(reduction="none", **ONEHOT)
    with pytest.raises(NotImplementedError, match="other_act"):
        pkg.DiceLoss(other_act=torch.tanh)
    for kw, name in ((dict(region="iou"), "region"), (dict(voxel="bce"), "voxel"), (dict(w_type="cubic"), "w_type"),
                     (dict(region="none", voxel="none"), "voxel"), (dict(softmax=True, sigmoid=True), "sigmoid"),
                     (dict(voxel="none", class_weight=[1.0], **ONEHOT), "class_weight"),
                     (dict(class_weight=[1.0, -1.0], **ONEHOT), "class_weight")):
        with pytest.raises(ValueError, match=name):
            S(**kw)
    # what DiceCELoss refuses is what SegLoss is for
    S(include_background=False, squared_pred=True, batch=True, lambda_region=0.5, lambda_voxel=2.0, region="jaccard", **ONEHOT)
    pkg.DiceLoss(jaccard=True, **MULTI), pkg.TverskyLoss(alpha=0.3, beta=0.7, **ONEHOT), pkg.GeneralizedDiceLoss(w_type="simple", **MULTI)
    pkg.FocalLoss(to_onehot_y=True, weight=[1.0, 2.0]), pkg.DiceFocalLoss(include_background=False, **ONEHOT)
    # shape errors come before any device work
    with pytest.raises(ValueError, match="include_background"):
        pkg.DiceLoss(include_background=False, **MULTI)(torch.zeros(1, 1, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4))
    with pytest.raises(ValueError, match="class_weight"):
        S(class_weight=[1.0, 2.0, 3.0], **ONEHOT)(torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4))
    with pytest.raises(ValueError):
        S(**ONEHOT)(torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 2, 4, 4, 4))
    with pytest.raises(ValueError):
        S(**MULTI)(torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4))


def test_no_cpu_fallback(pkg):
    for crit in (pkg.SegLoss(**ONEHOT), pkg.DiceFocalLoss(**ONEHOT), pkg.SegLoss(class_weight=[1.0, 2.0], **ONEHOT)):
        with pytest.raises(RuntimeError, match="ROCm device"):
            crit(torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4))
        with pytest.raises(RuntimeError, match="ROCm device"):
            crit.terms(torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4))


def test_abi_additions(pkg):
    txt = open(os.path.join(ROOT, "include", "unetr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for sym in ("unetr_segloss_fwd", "unetr_segloss_bwd", "unetr_segloss_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % sym, code), sym
        assert sym in pkg._capi.EXPORTED_SYMBOLS
    assert "unetr_segloss_desc" in code
    assert pkg._capi.ABI_VERSION == 21 and int(re.search(r"#define\s+UNETR_ABI_VERSION\s+(\d+)", txt).group(1)) == 21
    lib = pkg._capi.load()
    assert lib.unetr_abi_version() == 21
    # the struct the binding fills is the struct the header declares: same fields, same order
    body = re.search(r"typedef struct unetr_segloss_desc \{(.*?)\} unetr_segloss_desc;", code, flags=re.S).group(1)
    names = [n for n in re.findall(r"[A-Za-z_]\w*", body) if n not in ("const", "int", "long", "float")]
    assert names == [f[0] for f in pkg._capi.SegLossDesc._fields_]
    # the workspace a descriptor needs: partial rows of 3C+1 floats per 4096-voxel chunk, then 3 doubles per (b,c); 0 when refused
    d = pkg._capi.SegLossDesc(B=2, C=4, V=96 ** 3, region=1, voxel=1, include_background=1)
    assert lib.unetr_segloss_workspace_bytes(d) == 2 * 216 * 13 * 4 + 2 * 4 * 3 * 8
    d.C = 17
    assert lib.unetr_segloss_workspace_bytes(d) == 0
