"""GPU checks of HausdorffDistanceMetric (csrc/metrics.hip) and ConfusionMatrixMetric against the CPU restatements of
tests/metrics_ref.py: exact per-item, per-class distances for percentile=None, 1e-12 for percentiles, the fused argmax path,
the accumulate / aggregate protocol of the reference's validation_all_metrics (unetr_segmentation_3d.py:134-209)."""
import math

import pytest
import torch

import metrics_ref as R

pytestmark = pytest.mark.gpu


def _same(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)])


def _close(a, b, rtol=1e-12):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    if a.shape != b.shape or not torch.equal(torch.isnan(a), torch.isnan(b)) or not torch.equal(torch.isinf(a), torch.isinf(b)):
        return False
    ok = torch.isfinite(a)
    return torch.equal(a[torch.isinf(a)], b[torch.isinf(b)]) and bool(((a[ok] - b[ok]).abs() <= rtol * b[ok].abs()).all())


def _organs(B, C, shape, seed, dev):
    from tools.bench_metrics import onehot, synthetic_organs
    logits, labels = synthetic_organs(B, C, *shape, seed=seed, device=dev)
    return logits, labels, onehot(logits.argmax(1, keepdim=True), C), onehot(labels, C)


@pytest.mark.parametrize("B,C,shape", [(2, 4, (96, 96, 96)), (1, 3, (91, 109, 91)), (1, 14, (128, 128, 64))])
def test_hd_exact_on_organs(pkg, dev, B, C, shape):
    _, _, p, t = _organs(B, C, shape, seed=11, dev=dev)
    got = pkg.HausdorffDistanceMetric(include_background=True)(p, t)
    assert got.dtype == torch.float64 and got.shape == (B, C)
    assert _same(got, R.hd_torch(p, t, include_background=True))
    assert torch.isfinite(got).all()


def _edge_batch(dev):
    cases = R.hd_edge_cases() + R.hd_random_cases(12, seed=1)
    ps, ts = zip(*[R.as_onehot(pr, gt) for _, pr, gt in cases])
    return torch.cat(ps).to(dev), torch.cat(ts).to(dev)


def test_hd_edge_cases_and_options(pkg, dev):
    p, t = _edge_batch(dev)
    for kw in (dict(), dict(directed=True), dict(percentile=0)):
        got = pkg.HausdorffDistanceMetric(include_background=True, **kw)(p, t)
        assert _same(got, R.hd_torch(p, t, include_background=True, **kw)), kw
    got = pkg.HausdorffDistanceMetric()(p, t)                      # include_background=False (MONAI's default)
    assert got.shape == (p.shape[0], 1) and _same(got, R.hd_torch(p, t))
    for kw in (dict(percentile=95), dict(percentile=50, directed=True), dict(percentile=100)):
        got = pkg.HausdorffDistanceMetric(include_background=True, **kw)(p, t)
        assert _close(got, R.hd_torch(p, t, include_background=True, **kw)), kw
    names = [c[0] for c in R.hd_edge_cases()]
    got = pkg.HausdorffDistanceMetric()(p, t)[:, 0].cpu()
    assert math.isnan(got[names.index("both_empty")]) and math.isnan(got[names.index("empty_pred")])
    assert got[names.index("empty_gt")] == math.inf


def test_hd_percentile_on_organs(pkg, dev):
    _, _, p, t = _organs(2, 4, (96, 96, 96), seed=12, dev=dev)
    got = pkg.HausdorffDistanceMetric(include_background=True, percentile=95)(p, t)
    assert _close(got, R.hd_torch(p, t, include_background=True, percentile=95))


def test_hd_from_logits_lists_and_determinism(pkg, dev):
    g = torch.Generator(device=dev).manual_seed(3)
    B, C = 2, 4
    logits = torch.randint(0, 3, (B, C, 40, 36, 30), device=dev, generator=g).float()      # many exact ties
    labels = torch.randint(0, C, (B, 1, 40, 36, 30), device=dev, generator=g).float()
    labels[:, :, 5:25, 5:20, 5:20] = 2.0
    p = torch.nn.functional.one_hot(logits.argmax(1), C).permute(0, 4, 1, 2, 3).float()   # torch.argmax: first maximum
    t = torch.nn.functional.one_hot(labels.long()[:, 0], C).permute(0, 4, 1, 2, 3).float()
    for kw in (dict(), dict(percentile=95)):
        m = pkg.HausdorffDistanceMetric(include_background=True, **kw)
        a = m(logits, labels, from_logits=True)
        b = m(p, t)
        c = m([x for x in p], [x for x in t])
        d = m(logits, labels, from_logits=True)
        assert _same(a, b) and _same(b, c) and torch.equal(a, d), kw
    assert _same(pkg.HausdorffDistanceMetric(include_background=True)(p, t), R.hd_torch(p, t, include_background=True))


def test_hd_aggregate_accumulates(pkg, dev):
    p, t = _edge_batch(dev)
    chunks = [(p[:5], t[:5]), (p[5:12], t[5:12]), (p[12:], t[12:])]
    for red in ("mean", "mean_batch"):
        m = pkg.HausdorffDistanceMetric(include_background=True, reduction=red)
        for a, b in chunks:
            m(a, b)
        raw = torch.cat([R.hd_torch(a, b, include_background=True) for a, b in chunks])
        assert torch.isnan(raw).any() and torch.isinf(raw).any()
        assert _close(m.aggregate(), R.reduction_ref(raw, red)), red
        m.reset()
        m(p[5:], t[5:])
        assert _close(m.aggregate(), R.reduction_ref(R.hd_torch(p[5:], t[5:], include_background=True), red))


def test_confusion_matrix_metric(pkg, dev):
    _, _, p, t = _organs(2, 4, (48, 40, 36), seed=13, dev=dev)
    calls = [(p, t), (p[:1], t[:1]), ([x for x in t], [x for x in p])]       # batched, one item, lists (decollated)
    data = torch.cat([R.confusion_matrix_ref(p, t), R.confusion_matrix_ref(p[:1], t[:1]), R.confusion_matrix_ref(t, p)])
    for name, key in (("precision", "ppv"), ("sensitivity", "tpr")):
        for red in ("mean", "mean_batch"):
            for cs in (False, True):
                m = pkg.ConfusionMatrixMetric(include_background=True, reduction=red, get_not_nans=False, metric_name=name,
                                              compute_sample=cs)
                for a, b in calls:
                    m(y_pred=a, y=b)
                res = m.aggregate()
                assert isinstance(res, list) and len(res) == 1
                ref = R.reduction_ref(R.cm_metric_ref(key, data), red) if cs else R.cm_metric_ref(key, R.reduction_ref(data, red))
                assert res[0].shape == ((1,) if red == "mean" else (4,)), (name, red, cs)     # MONAI: [1] / [C]
                assert _close(res[0], ref.reshape(res[0].shape)), (name, red, cs)
    logits, labels, _, _ = _organs(2, 4, (48, 40, 36), seed=13, dev=dev)
    m = pkg.ConfusionMatrixMetric(metric_name=["precision", "recall"])
    assert torch.equal(m(logits, labels, from_logits=True), m(p, t))
    assert len(m.aggregate()) == 2


def test_validation_all_metrics_loop(pkg, dev):
    """the four metrics of validation_all_metrics on sliding-window outputs of the C1 model (the oracle's own predictions,
    so argmax near-ties cannot differ), as test_sliding_window_inference_and_dice_metric does"""
    from oracle.unetr_oracle import (OracleUNETR, oracle_dice_metric, oracle_post_label, oracle_post_pred,
                                     oracle_sliding_window_inference, synthetic_volume)
    cfg = dict(in_channels=1, out_channels=2, img_size=(32, 32, 32), feature_size=16, hidden_size=128, mlp_dim=512,
               num_heads=4, pos_embed="perceptron", norm_name="instance", res_block=True)
    torch.manual_seed(4)
    ref = OracleUNETR(**cfg)
    hip = pkg.UNETR(**cfg)
    hip.load_state_dict(ref.state_dict(), strict=True)
    hip = hip.to(dev).eval()
    hip.precision = "fp32"
    mets = {(kind, red): (pkg.DiceMetric(True, red) if kind == "dice" else
                          pkg.ConfusionMatrixMetric(include_background=True, reduction=red, get_not_nans=False,
                                                    metric_name=kind) if kind in ("precision", "sensitivity") else
                          pkg.HausdorffDistanceMetric(include_background=True, reduction=red, get_not_nans=False))
            for kind in ("dice", "precision", "sensitivity", "hsd") for red in ("mean", "mean_batch")}
    raws = {"dice": [], "cm": [], "hsd": []}
    for size, seed in ((48, 30), (40, 31)):
        x, y = synthetic_volume(2, 1, size, 2, seed=seed)
        with torch.no_grad():
            out_r = oracle_sliding_window_inference(x, (32, 32, 32), 4, lambda w: ref(w)[1])
        out_h = pkg.sliding_window_inference(x.to(dev), (32, 32, 32), 4, hip)
        assert out_h.shape == out_r.shape
        pr, lr = oracle_post_pred(out_r, 2), oracle_post_label(y, 2)
        pl, ll = [v for v in pr.to(dev)], [v for v in lr.to(dev)]       # decollate_batch + post_pred / post_label
        for (kind, red), m in mets.items():
            m(y_pred=pl, y=ll)
            agg = m.aggregate() if kind in ("dice", "hsd") else m.aggregate()[0]
            assert agg.numel() == (1 if red == "mean" else 2)
        raws["dice"].append(oracle_dice_metric(pr, lr, "mean")[0])
        raws["cm"].append(R.confusion_matrix_ref(pr, lr))
        raws["hsd"].append(R.hd_torch(pr, lr, include_background=True))
    cm = torch.cat(raws["cm"])
    for red in ("mean", "mean_batch"):
        assert torch.allclose(mets[("dice", red)].aggregate().cpu().double(),
                              R.reduction_ref(torch.cat(raws["dice"]).double(), red), atol=1e-6)
        for kind, key in (("precision", "ppv"), ("sensitivity", "tpr")):
            agg = mets[(kind, red)].aggregate()[0]
            assert _close(agg, R.cm_metric_ref(key, R.reduction_ref(cm, red)).reshape(agg.shape)), (kind, red)
        assert _close(mets[("hsd", red)].aggregate(), R.reduction_ref(torch.cat(raws["hsd"]), red))


def test_hd_large_from_logits(pkg, dev):
    """[1,14,256,256,160] from logits within the workspace bound; a few organ classes against reference (i) on their boxes"""
    B, C, shape = 1, 14, (256, 256, 160)
    from tools.bench_metrics import synthetic_organs
    logits, labels = synthetic_organs(B, C, *shape, seed=21, device=dev)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    got = pkg.HausdorffDistanceMetric(include_background=True)(logits, labels, from_logits=True).cpu()
    torch.cuda.synchronize()
    V = shape[0] * shape[1] * shape[2]
    bound = 8 * B * V + pkg.metrics.HD_SLOT_BUDGET_BYTES + (1 << 20)        # class words + group slots (+ boxes, output)
    assert torch.cuda.max_memory_allocated(dev) - before <= bound
    assert got.shape == (1, 14) and torch.isfinite(got).all()
    am = logits.argmax(1)[0]
    lab = labels[0, 0]
    for c in (1, 6, 13):
        ref = R.hd_pair_ref((am == c).cpu(), (lab == c).cpu())
        assert got[0, c].item() == ref, c
