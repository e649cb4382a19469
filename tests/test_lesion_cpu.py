"""CPU side of the instance-level metrics: the two reference forms of the lesion-wise semantics agree, the
model of the kernels' hash table behaves as a dict, and the public functions validate their arguments and refuse CPU tensors."""
import math

import numpy as np
import pytest
import torch

import lesion_ref as ref

SHAPE = (12, 14, 70)


def same_record(a, b):
    for k in ("n_gt", "n_tp", "n_fn", "n_fp", "n_pred", "n_tp_pred"):
        assert a[k] == b[k], k
    assert a["dice"] == b["dice"]                                   # float64, term by term
    for k in ("dice_sum", "lesion_dice", "precision", "recall", "f1"):
        assert a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])), k


@pytest.mark.parametrize("min_lesion_voxels", [0, 6])
@pytest.mark.parametrize("dilation", [0, 1, 3])
def test_loop_and_pair_table_agree(dilation, min_lesion_voxels):
    seen = dict(tp=0, fn=0, fp=0, merged=0, ignored=0)
    for seed in range(8):
        pred, gt = ref.lesion_case(SHAPE, 100 + seed, n_gt=7, n_spurious=4)
        for conn in (1, 3):
            a = ref.lesion_loop(pred, gt, dilation, 2, conn, min_lesion_voxels)
            b = ref.lesion_pairs(pred, gt, dilation, 2, conn, min_lesion_voxels)
            same_record(a, b)
            seen["tp"] += a["n_tp"]; seen["fn"] += a["n_fn"]; seen["fp"] += a["n_fp"]
            seen["merged"] += a["n_gt"] < ref.lesion_loop(pred, gt, 0, 2, conn)["n_gt"]
            seen["ignored"] += a["n_gt"] - a["n_tp"] - a["n_fn"]
    print(dilation, min_lesion_voxels, seen)
    assert seen["tp"] and seen["fn"] and seen["fp"]
    assert (seen["merged"] > 0) == (dilation > 0) and (seen["ignored"] > 0) == (min_lesion_voxels > 0)


def test_empty_planes():
    z = np.zeros((3, 4, 5), np.uint8)
    one = z.copy(); one[1, 1, 1] = 1
    for fn in (ref.lesion_loop, ref.lesion_pairs):
        r = fn(z, z)
        assert r["lesion_dice"] == 1.0 and math.isnan(r["precision"]) and math.isnan(r["recall"]) and math.isnan(r["f1"])
        r = fn(one, z)
        assert (r["n_fp"], r["lesion_dice"], r["precision"]) == (1, 0.0, 0.0) and math.isnan(r["recall"])
        r = fn(z, one)
        assert (r["n_fn"], r["lesion_dice"], r["recall"]) == (1, 0.0, 0.0) and math.isnan(r["precision"])
    assert math.isnan(ref.panoptic_brute(z, z)["pq"]) and ref.panoptic_brute(one, z)["pq"] == 0.0
    assert ref.panoptic_brute(one, one) == dict(tp=1, fp=0, fn=0, iou=[1.0], sq=1.0, rq=1.0, pq=1.0)


@pytest.mark.parametrize("max_pairs", [2, 4, 32])                    # 4, 8 and 64 slots
def test_hash_table_model_against_dict(max_pairs):
    slots = ref.table_slots(max_pairs)
    assert slots == {2: 4, 4: 8, 32: 64}[max_pairs]
    rng = np.random.default_rng(max_pairs)
    for distinct in sorted({1, max_pairs - 1, max_pairs, max_pairs + 1, slots - 1, slots, slots + 1, 2 * slots}):
        # labels as the kernels see them: up to 2^31 - 1, and pairs that collide in the low bits
        pairs = set()
        while len(pairs) < distinct:
            pairs.add((int(rng.integers(1, 2 ** 31)), int(rng.integers(1, 2 ** 31))) if rng.random() < 0.5
                      else (int(rng.integers(1, 4)), int(rng.integers(1, 2 ** 31))))
        runs = [(p, int(rng.integers(1, 65)), int(rng.integers(0, 2))) for p in pairs for _ in range(int(rng.integers(1, 5)))]
        want = {}
        for p, n, w in runs:
            e = want.setdefault(p, [0, 0])
            e[0] += n
            e[1] += n * w
        for order in range(4):
            rng.shuffle(runs)
            t = ref.PairTableModel(max_pairs)
            dropped = sum(not t.insert(ref.pack(*p), n, n * w) for p, n, w in runs)
            assert t.overflow == (distinct > max_pairs), (distinct, order)
            assert t.pairs == min(distinct, slots) and ref.probe_chains_closed(t.keys)
            got = t.as_dict()
            if distinct <= slots:
                assert dropped == 0 and got == want, (distinct, order)
            else:
                assert dropped > 0 and len(got) == slots and all(want[k][0] >= v[0] > 0 for k, v in got.items())


def test_hash_is_murmur3_finalizer():
    assert ref.hash64(0) == 0 and ref.hash64(1) == 0xb456bcfc34c2cb2c
    assert ref.table_slots(1) == 2 and ref.table_slots(65536) == 131072 and ref.table_slots(3) == 8


def test_argument_validation(pkg):
    L = pkg.lesion_metrics
    x = torch.zeros(1, 2, 4, 4, 4)
    for fn in (pkg.lesion_wise_metrics, pkg.panoptic_quality):
        with pytest.raises(ValueError, match="B,C,D,H,W"):
            fn(x[0], x[0])
        with pytest.raises(ValueError, match="same shape"):
            fn(x, torch.zeros(1, 2, 4, 4, 5))
        with pytest.raises(ValueError, match="float32"):
            fn(x.to(torch.uint8), x.to(torch.uint8))
        with pytest.raises(ValueError, match="class_ids"):
            fn(x, x, class_ids=2)
        with pytest.raises(ValueError, match="connectivity"):
            fn(x, x, connectivity=4)
        for bad in (0, -1, 1.5, True):
            with pytest.raises(ValueError, match="max_pairs"):
                fn(x, x, max_pairs=bad)
        with pytest.raises(NotImplementedError, match="max_pairs"):
            fn(x, x, max_pairs=2 ** 24 + 1)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="dilation"):
            pkg.lesion_wise_metrics(x, x, dilation=bad)
        with pytest.raises(ValueError, match="min_lesion_voxels"):
            pkg.lesion_wise_metrics(x, x, min_lesion_voxels=bad)
    for bad in (None, 0, 4):
        with pytest.raises(ValueError, match="connectivity"):
            pkg.lesion_wise_metrics(x, x, dilation_connectivity=bad)
    with pytest.raises(ValueError, match="metric_name"):
        pkg.LesionWiseMetric(metric_name="dice")
    with pytest.raises(NotImplementedError):
        pkg.LesionWiseMetric(reduction="sum")
    with pytest.raises(ValueError, match="dilation"):
        pkg.LesionWiseMetric(dilation=-1)
    a = torch.zeros(1, 4, 4, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="int32"):
        L.label_overlaps(a.long(), a.long())
    with pytest.raises(ValueError, match="same shape"):
        L.label_overlaps(a, a[:, :2])
    with pytest.raises(ValueError, match="mask"):
        L.label_overlaps(a, a, a)
    assert L.table_slots(65536) == ref.table_slots(65536) and L.table_slots(1) == 2 and L.table_slots(5) == 16


def test_no_cpu_fallback(pkg):
    x = torch.zeros(1, 2, 4, 4, 4)
    ids = torch.zeros(1, 1, 4, 4, 4, dtype=torch.uint8)
    a = torch.zeros(1, 4, 4, 4, dtype=torch.int32)
    for call in (lambda: pkg.lesion_wise_metrics(x, x), lambda: pkg.panoptic_quality(x, x),
                 lambda: pkg.lesion_wise_metrics(ids, ids, class_ids=3), lambda: pkg.LesionWiseMetric()(y_pred=[x[0]], y=[x[0]]),
                 lambda: pkg.lesion_metrics.label_overlaps(a, a)):
        with pytest.raises(RuntimeError, match="ROCm device"):
            call()


def test_exports_and_workspace(pkg):
    for name in ("lesion_wise_metrics", "LesionWiseMetric", "panoptic_quality"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(pkg.lesion_metrics, name)
    assert "unetr_label_overlaps" in pkg._capi.EXPORTED_SYMBOLS and "unetr_label_overlaps_workspace_bytes" in pkg._capi.EXPORTED_SYMBOLS
    assert pkg.lesion_metrics.LesionWiseMetrics._fields == ("n_gt", "n_tp", "n_fn", "n_fp", "n_pred", "dice_sum", "lesion_dice",
                                                            "precision", "recall", "f1", "overflow")
    ws = pkg._capi.load().unetr_label_overlaps_workspace_bytes
    D, H, W, mp = 5, 7, 67, 100
    V, slots = D * H * W, ref.table_slots(mp)
    sizes = [ws(D, H, W, mp, g) for g in range(5)]
    steps = {b - a for a, b in zip(sizes, sizes[1:])}
    assert sizes[0] == 0 or len(steps) <= 2                          # linear in the group up to the 256-byte rounding
    assert sizes[1] >= 16 * slots + 20 * V and sizes[1] < 16 * slots + 20 * V + 8 * 1024 + 10 * 256
    assert ws(1025, 1, 1, mp, 1) == 0 and ws(0, 4, 4, mp, 1) == 0 and ws(4, 4, 4, 0, 1) == 0 and ws(4, 4, 4, 2 ** 24 + 1, 1) == 0
