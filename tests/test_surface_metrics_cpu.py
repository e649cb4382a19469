"""CPU checks of the spacing-aware surface metrics' definitions: the scipy `sampling=` restatement and the float64 min-plus
restatement of tests/surface_ref.py agree on the seeded cases, the rejected arguments, Geometry.native_spacing() and the exports."""
import inspect
import math

import numpy as np
import pytest
import torch

import metrics_ref as R
import surface_ref as S

SPACINGS = ((5.0, 0.8, 0.8), (2.5, 0.7, 1.3), (1.5, 0.9765625, 0.9765625))
CASES = R.hd_edge_cases() + R.hd_random_cases(12, seed=1)


@pytest.mark.parametrize("spacing", SPACINGS)
def test_minplus_restatement_equals_scipy(spacing):
    pytest.importorskip("scipy")
    worst = 0.0
    for name, pred, gt in CASES:
        ep, eg = S.pair_edges(pred, gt)
        for a, b in ((ep, eg), (eg, ep)):
            d1, d2 = S.directed_scipy(a, b, spacing), S.directed_minplus(a, b, spacing)
            assert d1.shape == d2.shape and np.array_equal(np.isinf(d1), np.isinf(d2)), name
            ok = np.isfinite(d1)
            if ok.any():
                worst = max(worst, float(np.max(np.abs(d1[ok] - d2[ok]) / np.maximum(d1[ok], 1e-300))))
    assert worst <= 4 * np.finfo(np.float64).eps, worst     # the two differ by rounding in the sum of three squares only


def test_unit_spacing_restatement_equals_voxel_units():
    for name, pred, gt in CASES:
        rec = S.record_ref(pred, gt, percentiles=(95,), directed_fn=S.directed_minplus)
        for directed in (False, True):
            a, b = S.hd_ref(rec, directed=directed), R.hd_pair_ref(pred, gt, directed=directed)
            assert (math.isnan(a) and math.isnan(b)) or a == b, name
        a, b = S.hd_ref(rec, k=0), R.hd_pair_ref(pred, gt, percentile=95)
        assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-12 * abs(b), name


def test_nan_inf_rules():
    cases = {n: (p, g) for n, p, g in R.hd_edge_cases()}
    r = S.record_ref(*cases["empty_gt"], spacing=SPACINGS[0], percentiles=(50,), tau=1.0, directed_fn=S.directed_minplus)
    assert r["n_gt"] == 0 and r["max_pg"] == math.inf and r["mean_pg"] == math.inf and math.isnan(r["pct_pg"][0])
    assert math.isnan(r["max_gp"]) and math.isnan(r["mean_gp"]) and r["within_pg"] == 0
    assert S.asd_ref(r) == math.inf and math.isnan(S.asd_ref(r, symmetric=True)) and S.nsd_ref(r) == 0.0
    r = S.record_ref(*cases["both_empty"], tau=1.0, directed_fn=S.directed_minplus)
    assert math.isnan(S.nsd_ref(r)) and math.isnan(S.asd_ref(r)) and math.isnan(S.hd_ref(r))
    r = S.record_ref(*cases["empty_pred"], tau=1.0, directed_fn=S.directed_minplus)
    assert math.isnan(S.asd_ref(r)) and S.nsd_ref(r) == 0.0


def test_argument_errors(pkg):
    z = torch.zeros(1, 2, 4, 4, 4)
    for bad in ((1.0, 1.0), (1.0, 1.0, 1.0, 1.0)):
        with pytest.raises(ValueError, match="three"):
            pkg.surface_metrics(z, z, spacing=bad)
        with pytest.raises(ValueError, match="three"):
            pkg.HausdorffDistanceMetric(spacing=bad)
    for bad in ((1.0, 0.0, 1.0), (1.0, -2.0, 1.0), (1.0, math.inf, 1.0), (math.nan, 1.0, 1.0)):
        with pytest.raises(ValueError, match="positive and finite"):
            pkg.surface_metrics(z, z, spacing=bad)
        with pytest.raises(ValueError, match="positive and finite"):
            pkg.SurfaceDistanceMetric(spacing=bad)
        with pytest.raises(ValueError, match="positive and finite"):
            pkg.SurfaceDiceMetric([1.0], spacing=bad)(z, z)
    for bad in ((-1,), (50, 100.5)):
        with pytest.raises(ValueError, match="between 0 and 100"):
            pkg.surface_metrics(z, z, percentiles=bad)
    with pytest.raises(ValueError, match="between 0 and 100"):
        pkg.HausdorffDistanceMetric(percentile=101, spacing=(1, 1, 1))
    with pytest.raises(NotImplementedError, match="at most 8"):
        pkg.surface_metrics(z, z, percentiles=tuple(range(9)))
    for cls, args in ((pkg.SurfaceDistanceMetric, ()), (pkg.SurfaceDiceMetric, ([1.0],)), (pkg.HausdorffDistanceMetric, ())):
        with pytest.raises(NotImplementedError, match="euclidean"):
            cls(*args, distance_metric="chessboard")
        with pytest.raises(NotImplementedError, match="reduction"):
            cls(*args, reduction="sum")
        with pytest.raises(NotImplementedError, match="get_not_nans"):
            cls(*args, get_not_nans=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):         # arguments are checked first, then the device
        pkg.surface_metrics(z, z, spacing=(1, 1, 1))


def test_native_spacing(pkg):
    A = np.diag([0.8, 0.8, 5.0, 1.0])
    A[:3, 3] = (-90.0, 126.0, -72.0)
    g = pkg.preprocess.geometry((20, 24, 7), A, pixdim=(1.5, 1.5, 2.0))
    assert g.native_spacing() == (0.8, 0.8, 5.0) and g.pixdim == (1.5, 1.5, 2.0)
    A[:, 1] *= -1                                                       # a flipped axis: the size stays positive
    assert pkg.preprocess.geometry((20, 24, 7), A).native_spacing() == (0.8, 0.8, 5.0)
    P = A[:, [2, 0, 1, 3]]                                              # permuted axes: file order, not world order
    sp = pkg.preprocess.geometry((7, 20, 24), P).native_spacing()
    assert isinstance(sp, tuple) and sp == (5.0, 0.8, 0.8)


def test_exports_and_signatures(pkg):
    for name in ("surface_metrics", "SurfaceDistanceMetric", "SurfaceDiceMetric"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(pkg.metrics, name)
    p = inspect.signature(pkg.surface_metrics).parameters
    assert list(p) == ["y_pred", "y", "spacing", "include_background", "percentiles", "thresholds", "from_logits", "class_ids"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[2:])
    assert p["spacing"].default is None and p["percentiles"].default == () and p["include_background"].default is False
    p = inspect.signature(pkg.HausdorffDistanceMetric.__init__).parameters
    assert list(p)[1:] == ["include_background", "distance_metric", "percentile", "directed", "reduction", "get_not_nans", "spacing"]
    assert p["spacing"].default is None
    p = inspect.signature(pkg.SurfaceDistanceMetric.__init__).parameters
    assert list(p)[1:] == ["include_background", "symmetric", "distance_metric", "reduction", "get_not_nans", "spacing"]
    p = inspect.signature(pkg.SurfaceDiceMetric.__init__).parameters
    assert list(p)[1:] == ["class_thresholds", "include_background", "distance_metric", "reduction", "get_not_nans", "spacing"]
    assert {"unetr_surface_metrics", "unetr_surface_metrics_workspace_bytes"} <= set(pkg._capi.EXPORTED_SYMBOLS)
    lib = pkg._capi.load()
    V = 12 * 10 * 8
    base = lib.unetr_surface_metrics_workspace_bytes(2, 3, 12, 10, 8, 0, 0)
    assert base >= 2 * V * 8
    per = lib.unetr_surface_metrics_workspace_bytes(2, 3, 12, 10, 8, 1, 0) - base
    assert 17 * V <= per <= 17 * V + 8752 + 3 * 256                     # the header's formula (+ 256-byte alignment)
    assert lib.unetr_surface_metrics_workspace_bytes(2, 3, 12, 10, 8, 1, 3) - base - per == 32 * 1024
