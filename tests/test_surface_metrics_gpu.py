"""GPU checks of surface_metrics (csrc/metrics.hip, unetr_surface_metrics) and the classes over it -- HausdorffDistanceMetric
with a spacing, SurfaceDistanceMetric, SurfaceDiceMetric -- against the scipy `sampling=` restatement of tests/surface_ref.py:
rtol 1e-12 in float64 with identical nan / inf placement, exact edge and within-tolerance counts."""
import functools
import math

import numpy as np
import pytest
import torch

import metrics_ref as R
import surface_ref as S
from guard import Guard

pytestmark = pytest.mark.gpu

SPACINGS = ((5.0, 0.8, 0.8), (2.5, 0.7, 1.3), (1.5, 0.9765625, 0.9765625))
PCTS = (1, 50, 95, 100)
SCALARS = ("n_pred", "n_gt", "max_pg", "max_gp", "mean_pg", "mean_gp", "within_pg", "within_gp")


def _close(a, b, rtol=1e-12):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    if a.shape != b.shape or not torch.equal(torch.isnan(a), torch.isnan(b)) or not torch.equal(torch.isinf(a), torch.isinf(b)):
        return False
    ok = torch.isfinite(a)
    return torch.equal(a[torch.isinf(a)], b[torch.isinf(b)]) and bool(((a[ok] - b[ok]).abs() <= rtol * b[ok].abs()).all())


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int64), b.view(torch.int64))


def _records_equal(a, b):
    fields = [(getattr(a, k), getattr(b, k)) for k in SCALARS if getattr(a, k) is not None]
    fields += list(zip(a.pct_pg, b.pct_pg)) + list(zip(a.pct_gp, b.pct_gp))
    return len(a.pct_pg) == len(b.pct_pg) and all(_bits_equal(x, y) for x, y in fields)


def _onehot2(masks):
    """[B, 2, D, H, W] float one-hot of a list of bool masks (channel 0 = complement)"""
    m = torch.stack(masks)
    return torch.stack([~m, m], 1).float()


def _pairs(preds, gts):
    """the (pred, gt) masks of a [B, 2] include_background=True result, row-major"""
    return [(q, h) for p, g in zip(preds, gts) for q, h in ((~p, ~g), (p, g))]


def _ref_records(preds, gts, spacing, percentiles=(), taus=None):
    """record_ref of every (item, channel) pair; taus = (background, mask) tolerances"""
    return [S.record_ref(p, g, spacing, percentiles, None if taus is None else taus[k & 1])
            for k, (p, g) in enumerate(_pairs(preds, gts))]


def _field(recs, key, k=None):
    vals = [r[key] if k is None else r[key][k] for r in recs]
    return torch.tensor(vals, dtype=torch.float64).view(-1, 2)


def _check_record(got, recs, percentiles, with_tau, tag):
    for key in SCALARS:
        if key.startswith("within") and not with_tau:
            assert getattr(got, key) is None
            continue
        ref = _field(recs, key)
        g = getattr(got, key)
        assert g.dtype == torch.float64 and g.is_cuda
        if key.startswith(("n_", "within")):
            assert torch.equal(g.cpu(), ref), (tag, key)
        else:
            assert _close(g, ref), (tag, key, g.cpu(), ref)
    for k in range(len(percentiles)):
        assert _close(got.pct_pg[k], _field(recs, "pct_pg", k)), (tag, "pct_pg", percentiles[k])
        assert _close(got.pct_gp[k], _field(recs, "pct_gp", k)), (tag, "pct_gp", percentiles[k])


def _tau_margin(recs, taus):
    """smallest |d - tau| over the reference distances that are not exactly tau"""
    worst = math.inf
    for k, r in enumerate(recs):
        for d in (r["d_pg"], r["d_gp"]):
            d = d[np.isfinite(d)]
            off = np.abs(d - taus[k & 1])
            off = off[off > 0]
            if off.size:
                worst = min(worst, float(off.min()))
    return worst


@functools.lru_cache(maxsize=None)
def _edge_masks():
    cases = R.hd_edge_cases() + R.hd_random_cases(12, seed=1)
    return [c[1] for c in cases], [c[2] for c in cases]


@functools.lru_cache(maxsize=None)
def _edge_refs(spacing, percentiles, taus):
    preds, gts = _edge_masks()
    return _ref_records(preds, gts, spacing, percentiles, taus)


def _edge_batch(dev):
    preds, gts = _edge_masks()
    return _onehot2(preds).to(dev), _onehot2(gts).to(dev)


# ---------------------------------------------------------------- 1. edge and seeded cases vs scipy
@pytest.mark.parametrize("spacing", SPACINGS)
def test_edge_and_seeded_cases_vs_scipy(pkg, dev, spacing):
    p, t = _edge_batch(dev)
    taus = (1.0, 2.0)
    recs = _edge_refs(spacing, PCTS, taus)
    assert _tau_margin(recs, taus) >= 1e-9                  # the count comparison below is meaningful
    got = pkg.surface_metrics(p, t, spacing=spacing, include_background=True, percentiles=PCTS, thresholds=taus)
    _check_record(got, recs, PCTS, True, spacing)
    col = lambda fn: torch.tensor([fn(r) for r in recs], dtype=torch.float64).view(-1, 2)
    kw = dict(include_background=True, spacing=spacing)
    assert _close(pkg.HausdorffDistanceMetric(**kw)(p, t), col(S.hd_ref))
    assert _close(pkg.HausdorffDistanceMetric(directed=True, **kw)(p, t), col(lambda r: S.hd_ref(r, directed=True)))
    assert _close(pkg.HausdorffDistanceMetric(percentile=95, **kw)(p, t), col(lambda r: S.hd_ref(r, k=2)))
    assert _close(pkg.HausdorffDistanceMetric(percentile=50, directed=True, **kw)(p, t),
                  col(lambda r: S.hd_ref(r, k=1, directed=True)))
    assert _close(pkg.SurfaceDistanceMetric(**kw)(p, t), col(S.asd_ref))
    assert _close(pkg.SurfaceDistanceMetric(symmetric=True, **kw)(p, t), col(lambda r: S.asd_ref(r, symmetric=True)))
    nsd = pkg.SurfaceDiceMetric(taus, **kw)(p, t)
    assert _close(nsd, col(S.nsd_ref))
    names = [c[0] for c in R.hd_edge_cases()]
    one = pkg.SurfaceDistanceMetric(spacing=spacing)(p, t)[:, 0].cpu()          # include_background=False: the mask channel
    assert one.shape == (p.shape[0],) and math.isnan(one[names.index("empty_pred")]) and one[names.index("empty_gt")] == math.inf
    assert math.isnan(nsd[names.index("both_empty"), 1]) and nsd[names.index("empty_gt"), 1] == 0.0
    with pytest.raises(ValueError, match="one threshold per evaluated class"):
        pkg.SurfaceDiceMetric((1.0,), **kw)(p, t)


# ---------------------------------------------------------------- 2. NSD count boundary
def test_nsd_count_boundary(pkg, dev):
    p, t = _edge_batch(dev)
    for spacing in SPACINGS[:2]:
        for tau in (1.0, 2.0, 3.0):
            recs = _edge_refs(spacing, (), (tau, tau))
            assert _tau_margin(recs, (tau, tau)) >= 1e-9, (spacing, tau)
            got = pkg.surface_metrics(p, t, spacing=spacing, include_background=True, thresholds=(tau, tau))
            _check_record(got, recs, (), True, (spacing, tau))
    exact = 0
    for tau in (1.0, 2.0, 3.0):                             # unit spacing: many distances equal tau exactly, <= vs < shows
        recs = _edge_refs((1.0, 1.0, 1.0), (), (tau, tau))
        exact += sum(int((r[k] == tau).sum()) for r in recs for k in ("d_pg", "d_gp"))
        got = pkg.surface_metrics(p, t, spacing=(1, 1, 1), include_background=True, thresholds=(tau, tau))
        for key in ("within_pg", "within_gp", "n_pred", "n_gt"):
            assert torch.equal(getattr(got, key).cpu(), _field(recs, key)), (tau, key)
    assert exact > 100


# ---------------------------------------------------------------- 3. unit spacing reproduces the integer path
def test_unit_spacing_reproduces_integer_path(pkg, dev):
    p, t = _edge_batch(dev)
    for kw in (dict(), dict(directed=True), dict(percentile=0)):
        a = pkg.HausdorffDistanceMetric(include_background=True, spacing=(1, 1, 1), **kw)(p, t)
        b = pkg.HausdorffDistanceMetric(include_background=True, **kw)(p, t)
        assert _bits_equal(a, b), kw
    for kw in (dict(percentile=95), dict(percentile=50, directed=True), dict(percentile=100)):
        a = pkg.HausdorffDistanceMetric(include_background=True, spacing=(1, 1, 1), **kw)(p, t)
        b = pkg.HausdorffDistanceMetric(include_background=True, **kw)(p, t)
        assert _close(a, b), kw
    m = pkg.HausdorffDistanceMetric(include_background=True)                      # a spacing per call takes the new path too
    assert _bits_equal(m(p, t, spacing=(1, 1, 1)), m(p, t))
    assert _close(m(p, t, spacing=(2, 2, 2)), 2 * m(p, t))


# ---------------------------------------------------------------- 4. tile and loop boundaries
def _blob_pair(shape):
    c = [(n - 1) / 2 for n in shape]
    a = R._blob(shape, c, [0.47 * n for n in shape])
    b = R._blob(shape, [v + 0.06 * n for v, n in zip(c, shape)], [0.38 * n for n in shape])
    return a, b


def _six_faces(shape):
    a = torch.ones(shape, dtype=torch.bool)
    b = a.clone()
    b[3:-3, 5:-5, 4:-4] = False                              # a shell: both masks touch all six faces
    a[4:6, 8:12, 6:9] = False
    return a, b


@pytest.mark.parametrize("shape,maker,spacing", [((70, 9, 40), _blob_pair, (0.7, 5.0, 1.3)), ((9, 70, 33), _blob_pair, (5.0, 0.8, 0.8)),
                                                 ((10, 35, 18), _six_faces, (2.5, 0.7, 1.3))])
def test_tile_and_loop_boundaries(pkg, dev, shape, maker, spacing):
    a, b = maker(shape)
    assert a.any() and b.any()
    p, t = _onehot2([a]).to(dev), _onehot2([b]).to(dev)
    recs = _ref_records([a], [b], spacing, (50, 95), (1.0, 1.0))
    got = pkg.surface_metrics(p, t, spacing=spacing, include_background=True, percentiles=(50, 95), thresholds=(1.0, 1.0))
    assert min(r["n_pred"] for r in recs) > 0 and _tau_margin(recs, (1.0, 1.0)) >= 1e-9
    _check_record(got, recs, (50, 95), True, shape)


# ---------------------------------------------------------------- 5. select degeneracies
def test_select_degeneracies(pkg, dev):
    shape, spacing = (12, 40, 40), (2.5, 0.7, 1.3)
    z = lambda: torch.zeros(shape, dtype=torch.bool)
    blob = R._blob(shape, (6, 20, 20), (4, 12, 15))
    one = z(); one[2, 3, 4] = True
    two = z(); two[2, 3, 4] = True; two[9, 30, 33] = True
    plate_a = z(); plate_a[2] = True
    plate_b = z(); plate_b[6] = True
    plates2 = z(); plates2[0] = True; plates2[9] = True
    plate_c = z(); plate_c[3] = True
    preds, gts = [one, two, plate_a, plates2], [blob, blob, plate_b, plate_c]
    pcts = (0, 25, 50, 95, 99.5, 100)
    recs = _ref_records(preds, gts, spacing, pcts)
    mask = recs[1::2]
    assert [r["n_pred"] for r in mask[:2]] == [1.0, 2.0]
    assert len(np.unique(mask[2]["d_pg"])) == 1 and mask[2]["n_pred"] == 1600
    assert len(np.unique(mask[3]["d_pg"])) == 2 and mask[3]["n_pred"] == 3200
    p, t = _onehot2(preds).to(dev), _onehot2(gts).to(dev)
    got = pkg.surface_metrics(p, t, spacing=spacing, include_background=True, percentiles=pcts)
    _check_record(got, recs, pcts, False, "degenerate")
    assert _bits_equal(got.pct_pg[5], got.max_pg) and _bits_equal(got.pct_gp[5], got.max_gp)    # np.percentile(100) = max
    kw = dict(include_background=True, spacing=spacing)
    assert _bits_equal(pkg.HausdorffDistanceMetric(percentile=0, **kw)(p, t), pkg.HausdorffDistanceMetric(**kw)(p, t))   # MONAI: max


# ---------------------------------------------------------------- 6. input forms agree
def test_input_forms_agree(pkg, dev):
    from tools.bench_metrics import onehot, synthetic_organs
    B, C = 2, 4
    logits, labels = synthetic_organs(B, C, 24, 20, 28, seed=5, device=dev)
    ids = logits.argmax(1, keepdim=True)
    kw = dict(spacing=(5.0, 0.8, 0.8), percentiles=(50, 95), thresholds=(1.0, 2.0, 3.0, 4.0), include_background=True)
    a = pkg.surface_metrics(onehot(ids, C), onehot(labels, C), **kw)
    b = pkg.surface_metrics(logits, labels, from_logits=True, **kw)
    c = pkg.surface_metrics(ids.to(torch.uint8), labels.to(torch.uint8), class_ids=C, **kw)
    assert a.n_pred.shape == (B, C) and bool((a.n_pred > 0).all()) and bool(torch.isfinite(a.pct_pg[1]).all())
    assert _records_equal(a, b) and _records_equal(a, c)
    m = pkg.SurfaceDiceMetric((2.0, 3.0, 4.0), spacing=(5.0, 0.8, 0.8))
    assert _bits_equal(m(ids.to(torch.uint8), labels.to(torch.uint8), class_ids=C), m(logits, labels, from_logits=True))
    with pytest.raises(ValueError, match="uint8 class-id maps"):
        pkg.surface_metrics(ids.float(), labels, class_ids=C)


# ---------------------------------------------------------------- 7. groups
def test_slot_groups(pkg, dev, monkeypatch):
    p, t = _edge_batch(dev)
    B, C, D, H, W = p.shape
    kw = dict(spacing=SPACINGS[1], percentiles=(50, 95), thresholds=(1.0, 2.0), include_background=True)
    whole = pkg.surface_metrics(p, t, **kw)
    wb = pkg._capi.load().unetr_surface_metrics_workspace_bytes
    per_slot = wb(B, C, D, H, W, 1, 2) - wb(B, C, D, H, W, 0, 2)
    for slots in (1, 4):                                     # 54 pairs: 54 groups of 1; 13 groups of 4 and one of 2
        monkeypatch.setattr(pkg.metrics, "HD_SLOT_BUDGET_BYTES", slots * per_slot + per_slot // 2)
        assert _records_equal(pkg.surface_metrics(p, t, **kw), whole), slots


# ---------------------------------------------------------------- 8. determinism and memory discipline
def test_guarded_and_deterministic(pkg, dev):
    preds, gts = _edge_masks()
    kw = dict(spacing=SPACINGS[0], percentiles=PCTS, thresholds=(1.0, 2.0), include_background=True)
    with Guard(dev) as gd:                                   # inputs, output and workspace live between red zones; the
        p, t = _onehot2(preds).to(dev), _onehot2(gts).to(dev)   # workspace comes poisoned from torch.empty
        a = pkg.surface_metrics(p, t, **kw)
        b = pkg.surface_metrics(p, t, **kw)
        ids_p, ids_t = p[:, 1:].to(torch.uint8), t[:, 1:].to(torch.uint8)
        c = pkg.surface_metrics(ids_p, ids_t, class_ids=2, **kw)
        assert gd.check() > 0
    assert _records_equal(a, b) and _records_equal(a, c)
    _check_record(a, _edge_refs(SPACINGS[0], PCTS, (1.0, 2.0)), PCTS, True, "guarded")


# ---------------------------------------------------------------- 9. protocol
def test_protocol_lists_accumulation_aggregate(pkg, dev):
    p, t = _edge_batch(dev)
    spacing, taus = SPACINGS[1], (1.0, 2.0)
    recs = _edge_refs(spacing, PCTS, taus)
    col = lambda fn: torch.tensor([fn(r) for r in recs], dtype=torch.float64).view(-1, 2)
    chunks = [slice(0, 5), slice(5, 12), slice(12, None)]
    for red in ("mean", "mean_batch"):
        kw = dict(include_background=True, reduction=red, get_not_nans=False, spacing=spacing)
        for m, raw in ((pkg.HausdorffDistanceMetric(percentile=95, **kw), col(lambda r: S.hd_ref(r, k=2))),
                       (pkg.SurfaceDistanceMetric(symmetric=True, **kw), col(lambda r: S.asd_ref(r, symmetric=True))),
                       (pkg.SurfaceDiceMetric(taus, **kw), col(S.nsd_ref))):
            for k, sl in enumerate(chunks):
                if k == 1:
                    m(y_pred=[x for x in p[sl]], y=[x for x in t[sl]])           # decollated lists
                else:
                    m(y_pred=p[sl], y=t[sl])
            assert torch.isnan(raw).any()
            assert _close(m.aggregate(), R.reduction_ref(raw, red)), (type(m).__name__, red)
            m.reset()
            m(p[5:], t[5:])
            assert _close(m.aggregate(), R.reduction_ref(raw[5:], red)), (type(m).__name__, red)


def test_round_trip_on_the_native_grid(pkg, dev):
    """a restore_native(..., post="argmax") mask scored against a native label with spacing=geom.native_spacing()"""
    native = (20, 24, 7)
    A = np.diag([0.8, 0.8, 5.0, 1.0])
    geom = pkg.preprocess.geometry(native, A, pixdim=(1.0, 1.0, 1.0))
    assert geom.native_spacing() == (0.8, 0.8, 5.0)
    d, h, w = geom.crop_shape
    inside = R._blob((d, h, w), ((d - 1) / 2, (h - 1) / 2, (w - 1) / 2), (0.3 * d, 0.35 * h, 0.3 * w)).float()
    logits = torch.stack([1.0 - inside, inside]).to(dev)                          # [2, d, h, w] on the resampled grid
    mask = pkg.restore_native(logits, geom, mode="linear", post="argmax")       # uint8 [1, *native]
    label = R._blob(native, (9, 12, 3), (6, 7, 2.2)).to(torch.uint8)[None]
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (1, *native) and 0 < int(mask.sum()) < mask.numel()
    sp = geom.native_spacing()
    rec = S.record_ref(mask[0].cpu() == 1, label[0] == 1, sp, (95,), 2.0)
    assert _tau_margin([rec, rec], (2.0, 2.0)) >= 1e-9
    yp, yt = mask[None], label[None].to(dev)
    ref = lambda v: torch.tensor([[v]], dtype=torch.float64)
    assert _close(pkg.HausdorffDistanceMetric(percentile=95, spacing=sp)(yp, yt, class_ids=2), ref(S.hd_ref(rec, k=0)))
    assert _close(pkg.SurfaceDistanceMetric(symmetric=True, spacing=sp)(yp, yt, class_ids=2), ref(S.asd_ref(rec, symmetric=True)))
    assert _close(pkg.SurfaceDiceMetric((2.0,), spacing=sp)(yp, yt, class_ids=2), ref(S.nsd_ref(rec)))
    assert S.hd_ref(rec, k=0) != R.hd_pair_ref(mask[0].cpu() == 1, label[0] == 1, percentile=95)   # millimetres, not voxels
