"""CPU tests of the order statistics and the top-k loss: the float64 references (tests/topk_ref.py, tests/select_ref.py) against
torch's and numpy's own functions, the threshold-gap precondition of every GPU case, the constructors' refusals, and the C ABI
additions."""
import os
import re

import numpy as np
import pytest
import torch

from segloss_ref import segloss_ref
from select_ref import kth_ref, partition_value, percentile_ref
from topk_ref import case_gap, eager_topk, k_count, tie_weights, topk_ref, voxel_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONEHOT = dict(to_onehot_y=True, softmax=True)
MULTI = dict(to_onehot_y=False, sigmoid=True)


def _inputs(B, C, S, seed=0, multilabel=False):
    gen = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, C, S, S, S, generator=gen, dtype=torch.float64) * 2
    if multilabel:
        return logits, (torch.rand(B, C, S, S, S, generator=gen) < 0.35).double()
    return logits, torch.randint(0, C, (B, 1, S, S, S), generator=gen).double()


@pytest.mark.parametrize("k", [0.01, 10.0, 12.5, 33.0, 100.0])
def test_reference_is_the_eager_composition(pkg, k):
    """cross_entropy(reduction="none") -> torch.topk -> mean, value and (away from ties) gradient"""
    pkg.TopKLoss(k=k, **ONEHOT)
    logits, label = _inputs(2, 3, 7, seed=1)
    z1, z2 = logits.clone().requires_grad_(True), logits.clone().requires_grad_(True)
    X, want = topk_ref(z1, label, k=k, **ONEHOT), eager_topk(z2, label, k)
    assert abs(float((X - want).detach())) < 1e-12
    X.backward(), want.backward()
    assert (z1.grad - z2.grad).abs().max() < 1e-12


def test_k_100_is_the_cross_entropy_term(pkg):
    for kw, ml in ((ONEHOT, False), (MULTI, True)):
        logits, t = _inputs(2, 4, 6, seed=2, multilabel=ml)
        _, X = segloss_ref(logits, t, region="none", voxel="ce", **kw)
        assert abs(float(topk_ref(logits, t, k=100.0, **kw) - X)) < 1e-12


def test_weights_and_ignore_index_enter_the_values(pkg):
    w = [0.2, 1.0, 3.0, 0.5]
    pkg.TopKLoss(class_weight=w, ignore_index=255, **ONEHOT)
    logits, label = _inputs(2, 4, 6, seed=5)
    label[torch.rand(label.shape, generator=torch.Generator().manual_seed(6)) < 0.3] = 255
    u, valid = voxel_values(logits, label, class_weight=w, ignore_index=255)
    ce = torch.nn.functional.cross_entropy(logits, label[:, 0].long(), weight=torch.tensor(w, dtype=torch.float64), ignore_index=255,
                                           reduction="none").reshape(2, -1)
    assert int(valid.sum()) == int((label != 255).sum()) and (u[valid] - ce[valid]).abs().max() < 1e-12
    N = int(valid.sum())
    X = topk_ref(logits, label, k=20.0, class_weight=w, ignore_index=255, **ONEHOT)
    assert abs(float(X - torch.topk(ce[valid], k_count(N, 20.0)).values.mean())) < 1e-12


def test_tie_rule(pkg):
    """all values equal: every voxel weighs 1/N, whatever K; K inside a group: the group shares what is left of K"""
    u = torch.full((40,), 1.25, dtype=torch.float64)
    for K in (1, 7, 40):
        assert torch.equal(tie_weights(u, K), torch.full((40,), 1.0 / 40, dtype=torch.float64))
    u = torch.tensor([5.0, 3.0, 3.0, 3.0, 3.0, 1.0, 0.5], dtype=torch.float64)
    w = tie_weights(u, 3)                            # one value above the threshold 3.0, two of K left for four tied voxels
    assert w.tolist() == [1 / 3, 2 / 12, 2 / 12, 2 / 12, 2 / 12, 0.0, 0.0]
    assert abs(float((w * u).sum()) - float(torch.topk(u, 3).values.mean())) < 1e-15
    assert k_count(4913, 0.01) == 1 and k_count(4913, 10.0) == 491 and k_count(8, 100.0) == 8 and k_count(27648, 12.5) == 3456


def test_gpu_cases_keep_the_threshold_gap(pkg):
    """every (input, k) the GPU tests hold to the bounds: K-th and (K+1)-th largest reference value >= 1e-4 apart, relative"""
    import test_topk_gpu as T
    cases = T.gap_cases()
    assert len(cases) >= 30
    for cid, logits, target, k, kw in cases:
        gap = case_gap(logits, target, k, **kw)
        assert gap >= T.MIN_GAP, (cid, gap)
    # the two pairs the table excludes do fail it: the assertion has teeth
    from test_segloss_gpu import C3, inputs
    assert case_gap(*inputs(C3, "oh", None), 10.0, **ONEHOT) < T.MIN_GAP
    assert case_gap(*inputs(C3, "oh", "ignore"), 10.0, ignore_index=255, **ONEHOT) < T.MIN_GAP
    # the tie case cuts a group, by construction
    u, _ = voxel_values(*T.tie_inputs())
    assert case_gap(*T.tie_inputs(), 30.0, **ONEHOT) == 0.0 and len(set(u.reshape(-1).tolist())) <= 15


def test_select_reference(pkg):
    rng = np.random.default_rng(3)
    x = rng.standard_normal(501).astype(np.float32)
    x[:7] = [0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-40, x[20]]
    srt = np.sort(x)
    for r in (0, 1, 250, 499, 500):
        v, beyond, eq = kth_ref(x, r)
        assert v == srt[r] == partition_value(x, r) and beyond <= r < beyond + eq
        v, beyond, eq = kth_ref(x, r, largest=True)
        assert v == srt[500 - r] == partition_value(x, r, largest=True) and beyond <= r < beyond + eq
    v, beyond, eq = kth_ref(np.array([2.0, 1.0, 2.0, 3.0, 2.0], np.float32), 2)
    assert (v, beyond, eq) == (2.0, 1, 3)
    v, beyond, eq = kth_ref(np.array([2.0, 1.0, 2.0, 3.0, 2.0], np.float32), 0, largest=True)
    assert (v, beyond, eq) == (3.0, 0, 1)
    # -0 sorts below +0
    z = np.array([0.0, -0.0, 1.0], np.float32)
    assert np.signbit(kth_ref(z, 0)[0]) and not np.signbit(kth_ref(z, 1)[0]) and kth_ref(z, 1)[1:] == (1, 1)
    assert percentile_ref(np.arange(5, dtype=np.float32), 37.5) == 1.5


def test_constructor_refusals(pkg):
    T, D = pkg.TopKLoss, pkg.DiceTopKLoss
    for cls in (T, D):
        for k in (0.0, -1.0, 100.5, float("nan")):
            with pytest.raises(ValueError, match="k="):
                cls(k=k, **ONEHOT)
        for kw in (dict(), dict(to_onehot_y=True, sigmoid=True), dict(to_onehot_y=False, softmax=True), dict(reduction="sum", **ONEHOT),
                   dict(ignore_index=255, **MULTI), dict(class_weight=[1.0, 2.0], **MULTI)):
            with pytest.raises(NotImplementedError):
                cls(**kw)
        with pytest.raises(ValueError, match="sigmoid"):
            cls(softmax=True, sigmoid=True)
        with pytest.raises(ValueError, match="class_weight"):
            cls(class_weight=[1.0, -1.0], **ONEHOT)
        cls(k=100.0, **ONEHOT), cls(k=0.5, class_weight=[1.0, 2.0], ignore_index=-1, **ONEHOT), cls(**MULTI)
    with pytest.raises(NotImplementedError, match="other_act"):
        D(other_act=torch.tanh, **ONEHOT)
    with pytest.raises(NotImplementedError, match="squared_pred"):
        pkg.SegLoss(region="tversky", squared_pred=True, **ONEHOT)
    D(jaccard=True, squared_pred=True, batch=True, include_background=False, lambda_dice=0.5, lambda_topk=2.0, **ONEHOT)
    crit = T(**ONEHOT)
    with pytest.raises(ValueError, match="k="):
        crit.set_k(101.0)
    # shape errors come before any device work
    with pytest.raises(ValueError, match="class_weight"):
        T(class_weight=[1.0, 2.0, 3.0], **ONEHOT)(torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4))
    with pytest.raises(ValueError):
        T(**ONEHOT)(torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 2, 4, 4, 4))
    with pytest.raises(ValueError):
        T(**MULTI)(torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4))
    # SegLoss keeps its configuration: no voxel="topk"
    with pytest.raises(ValueError, match="voxel"):
        pkg.SegLoss(voxel="topk", **ONEHOT)


def test_no_cpu_fallback(pkg):
    for crit in (pkg.TopKLoss(**ONEHOT), pkg.DiceTopKLoss(**ONEHOT), pkg.TopKLoss(class_weight=[1.0, 2.0], **ONEHOT)):
        with pytest.raises(RuntimeError, match="ROCm device"):
            crit(torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4))
    with pytest.raises(RuntimeError, match="ROCm device"):
        pkg.kth_value(torch.zeros(8), 3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        pkg.percentile(torch.zeros(8), (0.5, 99.5))
    with pytest.raises(RuntimeError, match="ROCm device"):
        pkg.percentile(torch.zeros(2, 8), 50.0, channel_wise=True)


def test_abi_additions(pkg):
    txt = open(os.path.join(ROOT, "include", "unetr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for sym in ("unetr_select_kth", "unetr_select_workspace_bytes", "unetr_topkce_fwd", "unetr_topkce_bwd", "unetr_topkce_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % sym, code), sym
        assert sym in pkg._capi.EXPORTED_SYMBOLS
    assert pkg._capi.ABI_VERSION == 21 and int(re.search(r"#define\s+UNETR_ABI_VERSION\s+(\d+)", txt).group(1)) == 21
    lib = pkg._capi.load()
    assert lib.unetr_abi_version() == 21
    # the structs the binding fills are the structs the header declares: same fields, same order
    for name, cls in (("unetr_topkce_desc", pkg._capi.TopKCEDesc), ("unetr_select_result", pkg._capi.SelectResult)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), code, flags=re.S).group(1)
        names = [n for n in re.findall(r"[A-Za-z_]\w*", body) if n not in ("const", "int", "long", "float", "unsigned")]
        assert names == [f[0] for f in cls._fields_], name
    assert (pkg._capi.SELECT_LARGEST, pkg._capi.SELECT_PLAIN_HIST) == tuple(
        int(re.search(r"UNETR_SELECT_%s\s*=\s*(\d+)" % n, code).group(1)) for n in ("LARGEST", "PLAIN_HIST"))
    # the segloss descriptor did not move
    assert [f[0] for f in pkg._capi.SegLossDesc._fields_][:3] == ["B", "C", "V"] and len(pkg._capi.SegLossDesc._fields_) == 20
    # workspaces, as the header comment states them: the select's four 256-bin histograms + 16 state words; the loss's = that + 32
    # + one count per 1024-voxel block + one partial per 4096 values, rounded up to 16; 0 when refused
    assert lib.unetr_select_workspace_bytes(96 ** 3) == (4 * 256 + 16) * 4 == 4160
    assert lib.unetr_select_workspace_bytes(0) == 0 and lib.unetr_select_workspace_bytes(2 ** 31) == 0
    assert lib.unetr_select_workspace_bytes(2 ** 31 - 1) == 4160
    d = pkg._capi.TopKCEDesc(B=2, C=4, V=96 ** 3)
    assert lib.unetr_topkce_workspace_bytes(d) == 4160 + 32 + 4 * 2 * 864 + 4 * 432 == 12832
    d.V = 17 ** 3
    assert lib.unetr_topkce_workspace_bytes(d) == (4160 + 32 + 4 * 2 * 5 + 4 * 3 + 15) // 16 * 16
    d.C = 17
    assert lib.unetr_topkce_workspace_bytes(d) == 0
    d.C, d.multilabel, d.has_ignore = 4, 1, 1
    assert lib.unetr_topkce_workspace_bytes(d) == 0
