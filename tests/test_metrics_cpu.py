"""CPU checks of the validation metrics' definitions (HausdorffDistanceMetric, ConfusionMatrixMetric): the torch-only
restatement of the Hausdorff distance equals the recalled MONAI 0.6.0 code path on scipy, the confusion-matrix formula and
alias table, and the rejected arguments."""
import math

import pytest
import torch

import metrics_ref as R

PERCENTILES = (None, 0, 50, 95, 100)
CASES = R.hd_edge_cases() + R.hd_random_cases(40)


def _same(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)])


def test_hd_case_count():
    assert len(CASES) >= 50


@pytest.mark.parametrize("name,pred,gt", CASES, ids=[c[0] for c in CASES])
def test_hd_torch_reference_equals_scipy_restatement(name, pred, gt):
    pytest.importorskip("scipy")
    p, t = R.as_onehot(pred, gt)
    for pct in PERCENTILES:
        for directed in (False, True):
            a = R.hd_torch(p, t, include_background=True, percentile=pct, directed=directed)
            b = R.hd_monai_scipy(p, t, include_background=True, percentile=pct, directed=directed)
            assert _same(a, b), (name, pct, directed, a, b)
    a = R.hd_torch(p, t)                                   # include_background=False: the mask channel only
    assert a.shape == (1, 1) and _same(a, R.hd_monai_scipy(p, t))


def test_hd_edge_rules():
    """the squeeze rule and the nan / inf table, on the torch-only restatement"""
    cases = {n: (p, g) for n, p, g in R.hd_edge_cases()}
    ep, _ = R.edges_ref(cases["plate_3x3"][0], cases["plate_3x3"][1])
    assert int(ep.sum()) == 8                                # 1-thick 3x3 plate: the centre is not an edge
    ep, _ = R.edges_ref(*cases["single_voxel_both"])
    assert int(ep.sum()) == 0                                # 1x1x1 box: 0-d erosion keeps the voxel
    assert math.isnan(R.hd_pair_ref(*cases["both_empty"]))
    assert math.isnan(R.hd_pair_ref(*cases["empty_pred"]))   # d(P->G) = nan comes first in Python's max
    assert R.hd_pair_ref(*cases["empty_gt"]) == math.inf
    assert math.isnan(R.hd_pair_ref(*cases["empty_gt"], percentile=95))   # percentile of an all-inf array


def test_sq_edt_matches_brute_force():
    g = torch.Generator().manual_seed(3)
    feat = torch.rand(7, 6, 5, generator=g) > 0.9
    d = R.sq_edt_ref(feat)
    pts = feat.nonzero()
    grid = torch.stack(torch.meshgrid(*[torch.arange(n) for n in feat.shape], indexing="ij"), -1).reshape(-1, 1, 3)
    brute = ((grid - pts[None]) ** 2).sum(-1).min(1).values.reshape(feat.shape)
    assert torch.equal(d, brute)


def test_confusion_formulas_and_aliases(pkg):
    M = pkg.metrics
    cm = torch.tensor([[5.0, 3.0, 90.0, 2.0], [0.0, 0.0, 100.0, 0.0], [0.0, 4.0, 96.0, 0.0], [7.0, 0.0, 0.0, 1.0]],
                      dtype=torch.float64)
    for key, aliases in R.CM_ALIASES.items():
        ref = R.cm_metric_ref(key, cm)
        for name in aliases:
            assert M.confusion_metric_key(name) == key
            got = M.compute_confusion_matrix_metric(name, cm)
            assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(got[~torch.isnan(got)], ref[~torch.isnan(ref)])
    # hand-built values: precision 5/8, recall 5/7; zero denominators give nan
    assert M.compute_confusion_matrix_metric("precision", cm)[0].item() == 5 / 8
    assert M.compute_confusion_matrix_metric("sensitivity", cm)[0].item() == 5 / 7
    assert math.isnan(M.compute_confusion_matrix_metric("precision", cm)[1].item())
    assert math.isnan(M.compute_confusion_matrix_metric("recall", cm)[2].item())
    assert math.isnan(M.compute_confusion_matrix_metric("specificity", cm)[3].item())
    assert M.compute_confusion_matrix_metric("f1", cm)[0].item() == 10 / 15
    assert M.compute_confusion_matrix_metric("ppv", cm[0]).shape == (1,)
    with pytest.raises(NotImplementedError, match="sensitivity"):
        M.confusion_metric_key("matthews_correlation_coefficient")


def test_reduction_matches_reference(pkg):
    g = torch.Generator().manual_seed(5)
    f = torch.rand(4, 3, generator=g, dtype=torch.float64) * 10
    f[0, 1] = math.nan
    f[2, :] = math.nan
    f[3, 2] = math.inf
    for red in ("mean", "mean_batch"):
        got, ref = pkg.metrics.do_metric_reduction(f, red), R.reduction_ref(f, red)
        assert torch.allclose(got, ref, rtol=1e-12, atol=0, equal_nan=True), red
    assert pkg.metrics.do_metric_reduction(f, "mean").item() == math.inf
    assert pkg.metrics.do_metric_reduction(f, "mean_batch")[:2].isfinite().all()


def test_rejected_arguments(pkg):
    with pytest.raises(NotImplementedError):
        pkg.HausdorffDistanceMetric(distance_metric="chessboard")
    with pytest.raises(NotImplementedError):
        pkg.HausdorffDistanceMetric(get_not_nans=True)
    with pytest.raises(NotImplementedError):
        pkg.HausdorffDistanceMetric(reduction="sum")
    with pytest.raises(ValueError):
        pkg.HausdorffDistanceMetric(percentile=101)
    with pytest.raises(NotImplementedError):
        pkg.ConfusionMatrixMetric(get_not_nans=True)
    with pytest.raises(NotImplementedError):
        pkg.ConfusionMatrixMetric(reduction="none")
    with pytest.raises(NotImplementedError):
        pkg.ConfusionMatrixMetric(metric_name="balanced_accuracy")
    m = pkg.ConfusionMatrixMetric(metric_name=["precision", "Recall"])
    assert m.metric_name == ("precision", "Recall")


def test_cpu_tensors_raise(pkg):
    p, t = R.as_onehot(*R.hd_edge_cases()[0][1:])
    with pytest.raises(RuntimeError, match="ROCm device"):
        pkg.HausdorffDistanceMetric()(p, t)
    with pytest.raises(RuntimeError, match="ROCm device"):
        pkg.ConfusionMatrixMetric(metric_name="precision")(p, t)
