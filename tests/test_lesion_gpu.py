"""The instance-level metrics on the GPU against tests/lesion_ref.py (the literal per-lesion loop; brute-force panoptic quality).
Integers must be equal.  Float fields must lie within 2 n^2 2^-53 of the reference's math.fsum-based value, n = the lesions of
the plane: the worst-case reordering error of n terms in [0, 1] (each of the n - 1 additions of a partial sum <= n rounds by at
most n 2^-53); every other operation is a single correctly rounded division of exact integers on both sides."""
import math

import numpy as np
import pytest
import torch

import lesion_ref as ref
from guard import Guard

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 5, 7, 67), (2, 1, 17, 9, 130), (2, 3, 12, 14, 70)]
INTS = ("n_gt", "n_tp", "n_fn", "n_fp", "n_pred")
FLOATS = ("dice_sum", "lesion_dice", "precision", "recall", "f1")
U = 2.0 ** -53
ids = lambda s: "x".join(map(str, s))


def dev_t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).to(dev)


def lesion(pkg, dev, pred, gt, **kw):
    """lesion_wise_metrics on every channel; {field: numpy [B, C]}"""
    r = pkg.lesion_wise_metrics(dev_t(pred, dev), dev_t(gt, dev), include_background=True, **kw)
    for k in INTS + ("overflow",):
        assert getattr(r, k).dtype == torch.int64 and getattr(r, k).shape == pred.shape[:2]
    for k in FLOATS:
        assert getattr(r, k).dtype == torch.float64 and getattr(r, k).shape == pred.shape[:2]
    return {k: getattr(r, k).cpu().numpy() for k in r._fields}


def loop_records(pred, gt, dilation=3, dilation_connectivity=2, connectivity=None, min_lesion_voxels=0, **_):
    conn = 3 if connectivity is None else connectivity
    return [ref.lesion_loop(pred[b, c], gt[b, c], dilation, dilation_connectivity, conn, min_lesion_voxels)
            for b in range(pred.shape[0]) for c in range(pred.shape[1])]


def close(got, want, n):
    if math.isnan(want):
        return math.isnan(got)
    return abs(got - want) <= 2 * n * n * U


def check(got, records, planes=None):
    C = got["n_gt"].shape[1]
    for i, r in enumerate(records):
        if planes is not None and i not in planes:
            continue
        b, c = divmod(i, C)
        print(f"plane {i}: " + ", ".join(f"{k}={got[k][b, c]}/{r[k]}" for k in INTS) + " | " +
              ", ".join(f"{k}={got[k][b, c]!r}/{r[k]!r}" for k in FLOATS))
        for k in INTS:
            assert got[k][b, c] == r[k], (i, k)
        assert got["overflow"][b, c] == 0
        for k in FLOATS:
            assert close(float(got[k][b, c]), r[k], r["n_gt"]), (i, k, got[k][b, c], r[k])


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.int64), b[k].view(np.int64)) for k in a)


@pytest.mark.parametrize("dilation", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_random_against_loop(pkg, dev, shape, dilation):
    with Guard(dev) as gd:
        for mlv in (0, 6):
            pred, gt, records = ref.picked_planes(shape, dilation, mlv)
            assert all(r["n_gt"] >= 2 and r["n_fp"] >= 1 for r in records)
            got = lesion(pkg, dev, pred, gt, dilation=dilation, min_lesion_voxels=mlv)
            check(got, records)
            assert same_bits(got, lesion(pkg, dev, pred, gt, dilation=dilation, min_lesion_voxels=mlv))
        kw = dict(dilation=2, dilation_connectivity=1, connectivity=1)
        check(lesion(pkg, dev, pred, gt, **kw), loop_records(pred, gt, **kw))
        check(lesion(pkg, dev, pred, gt, dilation=0), loop_records(pred, gt, dilation=0))
    assert gd.check() > 0


def test_multilabel_background_and_class_ids(pkg, dev):
    shape = SHAPES[2]
    pred, gt, _ = ref.picked_planes(shape, 1, 0)
    r = pkg.lesion_wise_metrics(dev_t(pred * 3, dev), dev_t(gt * 0.5, dev), dilation=1)      # set where non-zero; channel 0 dropped
    assert r.lesion_dice.shape == (2, 2)
    check({k: getattr(r, k).cpu().numpy() for k in r._fields}, loop_records(pred[:, 1:], gt[:, 1:], dilation=1))
    ids_p = np.where(pred[:, 2:3] != 0, 2, pred[:, 1:2]).astype(np.uint8)                     # class-id maps of 3 classes
    ids_g = np.where(gt[:, 2:3] != 0, 2, gt[:, 1:2]).astype(np.uint8)
    r = pkg.lesion_wise_metrics(torch.from_numpy(ids_p).to(dev), torch.from_numpy(ids_g).to(dev), class_ids=3, dilation=1)
    onehot = lambda m: np.stack([m[:, 0] == 1, m[:, 0] == 2], axis=1).astype(np.uint8)
    check({k: getattr(r, k).cpu().numpy() for k in r._fields}, loop_records(onehot(ids_p), onehot(ids_g), dilation=1))


def vol(W=67, D=6, H=8):
    return np.zeros((1, 1, D, H, W), np.uint8)


def test_bridging_component_counts_for_both_lesions(pkg, dev):
    gt, pred = vol(), vol()
    gt[0, 0, 2, 3, 5:7] = 1
    gt[0, 0, 2, 3, 40:43] = 1
    pred[0, 0, 2, 3, 6:41] = 1                                      # one component, meets both
    got = lesion(pkg, dev, pred, gt, dilation=1)
    check(got, loop_records(pred, gt, dilation=1))
    assert [int(got[k][0, 0]) for k in INTS] == [2, 2, 0, 0, 1]
    assert got["dice_sum"][0, 0] == 2 * 1 / (35 + 2) + 2 * 1 / (35 + 3)


def test_dilation_merges_components_four_voxels_apart(pkg, dev):
    gt, pred = vol(), vol()
    gt[0, 0, 2, 3, 10] = 1
    gt[0, 0, 2, 3, 14] = 1
    pred[0, 0, 2, 3, 10] = 1
    for dilation, n_gt, n_fn in ((3, 1, 0), (1, 2, 1)):
        got = lesion(pkg, dev, pred, gt, dilation=dilation)
        check(got, loop_records(pred, gt, dilation=dilation))
        assert (got["n_gt"][0, 0], got["n_fn"][0, 0]) == (n_gt, n_fn)
    assert lesion(pkg, dev, pred, gt, dilation=3)["dice_sum"][0, 0] == 2 * 1 / (1 + 2)


def test_match_in_the_dilated_rim_only(pkg, dev):
    gt, pred = vol(), vol()
    gt[0, 0, 2, 3, 10] = 1
    pred[0, 0, 2, 3, 12] = 1
    got = lesion(pkg, dev, pred, gt)
    check(got, loop_records(pred, gt))
    assert [int(got[k][0, 0]) for k in INTS] == [1, 1, 0, 0, 1]     # a match with Dice 0: TP, not FN, and no FP
    assert got["dice_sum"][0, 0] == 0.0 and got["lesion_dice"][0, 0] == 0.0 and got["f1"][0, 0] == 1.0


def test_empty_planes(pkg, dev):
    gt, pred = np.zeros((2, 1, 6, 8, 67), np.uint8), np.zeros((2, 1, 6, 8, 67), np.uint8)
    pred[0, 0, 1, 1, 3] = pred[0, 0, 4, 6, 60:66] = 1              # item 0: empty ground truth, two predictions; item 1: both empty
    got = lesion(pkg, dev, pred, gt)
    check(got, loop_records(pred, gt))
    assert [int(got[k][0, 0]) for k in INTS] == [0, 0, 0, 2, 2] and got["lesion_dice"][0, 0] == 0.0
    assert got["precision"][0, 0] == 0.0 and math.isnan(got["recall"][0, 0]) and math.isnan(got["f1"][0, 0])
    assert [int(got[k][1, 0]) for k in INTS] == [0, 0, 0, 0, 0] and got["lesion_dice"][1, 0] == 1.0
    assert all(math.isnan(got[k][1, 0]) for k in ("precision", "recall", "f1"))


def test_ignored_lesion_and_its_match(pkg, dev):
    gt, pred = vol(), vol()
    gt[0, 0, 1, 1, 5] = 1                                           # one voxel: ignored under min_lesion_voxels=2
    pred[0, 0, 1, 1, 5:7] = 1                                       # its match: not a false positive
    gt[0, 0, 4, 5, 40:46] = 1
    pred[0, 0, 4, 5, 42:48] = 1
    got = lesion(pkg, dev, pred, gt, min_lesion_voxels=2, dilation=1)
    check(got, loop_records(pred, gt, min_lesion_voxels=2, dilation=1))
    assert [int(got[k][0, 0]) for k in INTS] == [2, 1, 0, 0, 2]
    assert got["precision"][0, 0] == 1.0 and got["lesion_dice"][0, 0] == 2 * 4 / 12
    assert lesion(pkg, dev, pred, gt, dilation=1)["n_tp"][0, 0] == 2


def read_tables(pkg, ws, planes, max_pairs):
    """[(keys uint64 [slots], values [slots, 2])] per plane from the head of the workspace (include/unetr_hip.h)"""
    slots = pkg.lesion_metrics.table_slots(max_pairs)
    raw = ws.cpu().numpy()
    al = lambda n: (n + 255) & ~255
    keys = raw[:planes * slots * 8].view(np.uint64).reshape(planes, slots)
    vals = raw[al(planes * slots * 8):al(planes * slots * 8) + planes * slots * 8].view(np.int32).reshape(planes, slots, 2)
    return [(keys[p], vals[p]) for p in range(planes)]


@pytest.mark.parametrize("W", [67, 130])
def test_runs_across_the_lane_boundary(pkg, dev, W):
    """x-stripes: the pair changes at x = 63 / 64 in one map and runs straight through that boundary in the other; rows do not
    start on 64-lane boundaries (W is odd or not a multiple of 64) and the last segment of a row is partial"""
    D, H = 3, 5
    x = np.arange(W)
    a = np.broadcast_to(1 + x // 64, (2, D, H, W)).astype(np.int32).copy()          # changes at 63 / 64 (and 127 / 128)
    b = np.broadcast_to(1 + (x + 10) // 50, (2, D, H, W)).astype(np.int32).copy()   # runs through 63 / 64
    a[1] = 7                                                                        # plane 1: one run per row, split by the waves
    b[1, :, :, :3] = 0
    a[0, 1, 2, 60:66] = 0                                                           # a hole over the boundary
    mask = (np.random.default_rng(W).random(a.shape) < 0.5).astype(np.float32)
    mask[0, 0, 0, 40:] = 1
    for m in (None, mask):
        counts, values, ws = pkg.lesion_metrics.label_overlaps(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev),
                                                               None if m is None else torch.from_numpy(m).to(dev),
                                                               max_pairs=16, return_workspace=True)
        for p, (keys, vals) in enumerate(read_tables(pkg, ws, 2, 16)):
            want = ref.pair_dict(a[p], b[p], None if m is None else m[p])
            assert ref.table_as_dict(keys, vals) == want and ref.probe_chains_closed(keys)
            assert counts[p, 7].item() == len(want) and counts[p, 6].item() == 0
    gt, pred = vol(W), vol(W)                                                        # and through the public function
    gt[0, 0, 2, 3, 50:W] = 1
    pred[0, 0, 2, 3, 58:W - 1] = 1
    pred[0, 0, 2, 4, 0:W] = 1
    got = lesion(pkg, dev, pred, gt, dilation=0)
    check(got, loop_records(pred, gt, dilation=0))
    assert got["dice_sum"][0, 0] == 2 * (W - 59) / ((W - 59 + W) + (W - 50))


def five_lesions():
    gt, pred = np.zeros((2, 1, 6, 8, 67), np.uint8), np.zeros((2, 1, 6, 8, 67), np.uint8)
    for k in range(5):                                              # item 0: five lesions, each with its own component
        gt[0, 0, 2, 3, 4 + 12 * k:7 + 12 * k] = 1
        pred[0, 0, 2, 3, 5 + 12 * k:8 + 12 * k] = 1
    gt[1, 0, 1, 2, 10:14] = 1                                       # item 1: two pairs and a spurious component
    pred[1, 0, 1, 2, 11:14] = 1
    gt[1, 0, 4, 5, 30:33] = 1
    pred[1, 0, 4, 5, 30:32] = 1
    pred[1, 0, 4, 1, 60] = 1
    return pred, gt


def test_overflow_flags_that_plane_only(pkg, dev):
    pred, gt = five_lesions()
    records = loop_records(pred, gt, dilation=1)
    assert (records[0]["n_tp"], records[1]["n_tp"], records[1]["n_fp"]) == (5, 2, 1)
    got = lesion(pkg, dev, pred, gt, dilation=1, max_pairs=2)        # 4 slots: item 0 fills the table and drops a pair
    assert got["overflow"].tolist() == [[1], [0]]
    assert all(math.isnan(got[k][0, 0]) for k in FLOATS)
    assert (got["n_gt"][0, 0], got["n_pred"][0, 0]) == (5, 5) and got["n_tp"][0, 0] == got["n_fn"][0, 0] == got["n_fp"][0, 0] == -1
    check(got, records, planes={1})
    for max_pairs in (4, 3):                                         # 8 slots hold the five pairs, yet more than max_pairs: flagged
        got = lesion(pkg, dev, pred, gt, dilation=1, max_pairs=max_pairs)
        assert got["overflow"].tolist() == [[1], [0]] and math.isnan(got["lesion_dice"][0, 0])
        check(got, records, planes={1})
    check(lesion(pkg, dev, pred, gt, dilation=1, max_pairs=5), records)


def test_exactly_max_pairs_does_not_overflow(pkg, dev):
    gt, pred = vol(130), vol(130)
    for k in range(8):
        gt[0, 0, 1 + (k % 2) * 3, 3, 4 + 15 * k:8 + 15 * k] = 1
        pred[0, 0, 1 + (k % 2) * 3, 3, 5 + 15 * k:10 + 15 * k] = 1
    records = loop_records(pred, gt, dilation=1)
    assert records[0]["n_tp"] == 8 and records[0]["n_pred"] == 8
    got = lesion(pkg, dev, pred, gt, dilation=1, max_pairs=8)        # 16 slots, half full: chains form
    check(got, records)
    assert got["overflow"][0, 0] == 0


def test_pair_table_of_one_voxel_components(pkg, dev):
    """a 3-D checkerboard (every voxel its own component under 6-connectivity) against slabs: many distinct pairs inserted at
    once, one counter that every inserting thread increments"""
    D, H, W = 6, 6, 66
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    checker = ((z + y + x) % 2 == 0).astype(np.float32)[None, None]
    slabs = (y % 2 == 0).astype(np.float32)[None, None]
    A = pkg.connected_components(dev_t(checker, dev), connectivity=1)[0]
    Bm = pkg.connected_components(dev_t(slabs, dev), connectivity=1)[0]
    a, b = A.cpu().numpy(), Bm.cpu().numpy()
    assert len(np.unique(a)) == 1 + D * H * W // 2
    mask = (np.random.default_rng(5).random(a.shape) < 0.5).astype(np.float32)
    want = ref.pair_dict(a[0], b[0], mask[0])
    assert len(want) > 500
    for max_pairs in (1024, len(want)):
        counts, _, ws = pkg.lesion_metrics.label_overlaps(A, Bm, torch.from_numpy(mask).to(dev), max_pairs=max_pairs,
                                                          return_workspace=True)
        (keys, vals), = read_tables(pkg, ws, 1, max_pairs)
        got = ref.table_as_dict(keys, vals)
        assert {(i, j, n, m) for (i, j), (n, m) in got.items()} == {(i, j, n, m) for (i, j), (n, m) in want.items()}
        assert ref.probe_chains_closed(keys)
        assert counts[0, 7].item() == len(want) and counts[0, 6].item() == 0
    counts, values = pkg.lesion_metrics.label_overlaps(A, Bm, max_pairs=len(want) - 1)
    assert counts[0, 6].item() == 1 and counts[0, 7].item() == len(want) and torch.isnan(values[0, :5]).all()


def panoptic(pkg, dev, pred, gt, **kw):
    r = pkg.panoptic_quality(dev_t(pred, dev), dev_t(gt, dev), include_background=True, **kw)
    return {k: getattr(r, k).cpu().numpy() for k in r._fields}


def check_panoptic(got, pred, gt, conn=3):
    seen = 0
    C = pred.shape[1]
    for i in range(pred.shape[0] * C):
        b, c = divmod(i, C)
        r = ref.panoptic_brute(pred[b, c], gt[b, c], conn)
        print(f"plane {i}: " + ", ".join(f"{k}={got[k][b, c]!r}/{r[k]!r}" for k in ("tp", "fp", "fn", "sq", "rq", "pq")))
        for k in ("tp", "fp", "fn"):
            assert got[k][b, c] == r[k], (i, k)
        assert got["overflow"][b, c] == 0
        for k in ("sq", "rq", "pq"):
            assert close(float(got[k][b, c]), r[k], max(r["tp"], 1)), (i, k)
        seen += r["tp"]
    return seen


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_panoptic_against_brute_force(pkg, dev, shape):
    pred, gt, _ = ref.picked_planes(shape, 1, 0)
    got = panoptic(pkg, dev, pred, gt)
    matches = check_panoptic(got, pred, gt)
    matches += check_panoptic(panoptic(pkg, dev, pred, gt, connectivity=1), pred, gt, 1)
    assert matches > 0
    assert same_bits(got, panoptic(pkg, dev, pred, gt))


def test_panoptic_threshold_is_exact(pkg, dev):
    gt, pred = np.zeros((2, 1, 6, 8, 67), np.uint8), np.zeros((2, 1, 6, 8, 67), np.uint8)
    gt[0, 0, 1, 1, 0:30] = 1
    pred[0, 0, 1, 1, 10:40] = 1                                     # n = 20, union 40: IoU exactly 1/2, no match
    gt[0, 0, 4, 5, 0:31] = 1
    pred[0, 0, 4, 5, 10:41] = 1                                     # n = 21, union 41: just above, a match
    got = panoptic(pkg, dev, pred, gt)
    check_panoptic(got, pred, gt)
    assert (got["tp"][0, 0], got["fp"][0, 0], got["fn"][0, 0]) == (1, 1, 1)
    assert got["sq"][0, 0] == 21 / 41 and got["rq"][0, 0] == 0.5 and got["pq"][0, 0] == (21 / 41) * 0.5
    assert all(math.isnan(got[k][1, 0]) for k in ("sq", "rq", "pq")) and got["tp"][1, 0] == 0      # item 1: empty / empty


@pytest.mark.parametrize("name", ["lesion_dice", "f1", "precision", "recall"])
def test_metric_class(pkg, dev, name):
    shape = SHAPES[2]
    pred, gt, records = ref.picked_planes(shape, 1, 0)
    pred2, gt2 = pred[::-1, ::-1].copy(), gt[::-1, ::-1].copy()
    records2 = loop_records(pred2, gt2, dilation=1)
    want = torch.tensor([r[name] for r in records + records2], dtype=torch.float64).view(4, 3)
    tol = max(2 * r["n_gt"] ** 2 for r in records + records2) * U + 8 * U
    for reduction in ("mean", "mean_batch"):
        metric = pkg.LesionWiseMetric(metric_name=name, include_background=True, reduction=reduction, dilation=1)
        first = metric(y_pred=dev_t(pred, dev), y=dev_t(gt, dev))
        second = metric(y_pred=list(dev_t(pred2, dev)), y=list(dev_t(gt2, dev)))                # a decollated list
        assert first.shape == second.shape == (2, 3)
        direct = pkg.lesion_wise_metrics(dev_t(pred2, dev), dev_t(gt2, dev), include_background=True, dilation=1)
        assert torch.equal(second.view(torch.int64), getattr(direct, name).view(torch.int64))
        got = metric.aggregate().cpu()
        ref_red = pkg.metrics.do_metric_reduction(want, reduction)
        print(name, reduction, got.tolist(), ref_red.tolist())
        assert got.shape == ref_red.shape and torch.allclose(got, ref_red, rtol=0, atol=tol)
        metric.reset()
        assert metric._buf == []


def test_graph_capture(pkg, dev):
    shape = SHAPES[1]
    pred_a, gt_a, _ = ref.picked_planes(shape, 3, 0)
    pred_b, gt_b = pred_a[::-1].copy(), gt_a[::-1].copy()           # other contents: the items swapped, part of one prediction gone
    pred_b[0, :, :8] = 0
    run =lambda p, g: torch.stack([t.to(torch.float64) for t in pkg.lesion_wise_metrics(p, g, include_background=True)] +
                                   [t.to(torch.float64) for t in pkg.panoptic_quality(p, g, include_background=True)])
    A, B = (dev_t(pred_a, dev), dev_t(gt_a, dev)), (dev_t(pred_b, dev), dev_t(gt_b, dev))
    eager_a, eager_b = run(*A), run(*B)
    bits = lambda t: t.view(torch.int64)
    assert not torch.equal(bits(eager_a), bits(eager_b))
    sp, sg = A[0].clone(), A[1].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(sp, sg)                                                  # warm-up: library load, allocator
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = run(sp, sg)
    for (p, g), eager in ((B, eager_b), (A, eager_a)):
        sp.copy_(p)
        sg.copy_(g)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(eager))
