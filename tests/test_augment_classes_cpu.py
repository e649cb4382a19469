"""CPU checks of class-balanced crop sampling: the C ABI's new symbols, what RandCropAugment refuses before any device work,
and the anchors of tests/augment_classes_ref.py, the restatement the GPU tests pin csrc/augment.hip's class kernels to."""
import math
import os
import re

import numpy as np
import pytest
import torch

import augment_classes_ref as K
import augment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("unetr_aug_class_ws_ints", "unetr_aug_class_count", "unetr_aug_class_scatter", "unetr_aug_sample_classes")
FREQ_SEED = 2024            # the seed of the frequency check below and of the GPU sampler tests, which replay this reference
FREQ_RATIOS = [0, 1, 2, 1, 3]


def _labels(shape, ncls, seed, absent=()):
    rng = np.random.default_rng(seed)
    lbl = rng.integers(0, ncls, size=(1, *shape))
    for c in absent:
        lbl[lbl == c] = 0
    return lbl


def _cfg(S, B, ns, seed):
    return dict(spatial_size=S, sampling="label_classes", pos_ratio=0.5, flip_prob=(0.3, 0.5, 0.7), rot90_prob=0.5, max_k=3,
                shift_prob=0.5, shift_range=(-0.1, 0.1), num_samples=ns, batch_size=B, seed=seed)


def test_exports_and_abi(pkg):
    assert pkg._capi.ABI_VERSION == 21
    header = open(os.path.join(ROOT, "include", "unetr_hip.h")).read()
    assert int(re.search(r"#define\s+UNETR_ABI_VERSION\s+(\d+)", header).group(1)) == 21
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for s in NEW_SYMBOLS:
        assert s in pkg._capi.EXPORTED_SYMBOLS, s
        assert re.search(r"\b%s\s*\(" % s, code), s
    assert "label_classes" in pkg.augment.SAMPLING_MODES and "weighted" not in pkg.augment.SAMPLING_MODES
    assert pkg.augment.SAMPLING_MODES[:2] == ("pos_neg", "uniform")          # the descriptor's 0 and 1 do not move


def test_construction_errors_before_any_device_work(pkg):
    class One:
        shapes = [(1, 1, 12, 12, 12)]

    class Three:
        shapes = [(1, 3, 12, 12, 12)]
    kw = dict(spatial_size=8, num_samples=2, sampling="label_classes")
    with pytest.raises(ValueError, match="num_classes is required"):
        pkg.RandCropAugment(One(), **kw)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="num_classes must be in 1..32"):
            pkg.RandCropAugment(One(), num_classes=bad, **kw)
    with pytest.raises(ValueError, match="num_classes must be None or 3"):
        pkg.RandCropAugment(Three(), num_classes=4, **kw)
    for extra in (dict(num_classes=5), dict(class_ratios=[1, 1]), dict(class_image_mask=True)):
        with pytest.raises(ValueError, match='belong to sampling="label_classes"'):
            pkg.RandCropAugment(One(), spatial_size=8, num_samples=2, **extra)


def test_lists_equal_a_direct_nonzero_loop():
    rng = np.random.default_rng(0)
    lbl = rng.integers(0, 7, size=(1, 5, 6, 7))                   # ids 5 and 6 are >= num_classes: in no list
    img = rng.standard_normal((2, 5, 6, 7)).astype(np.float32)
    img[rng.random(img.shape) < 0.4] = 0.0
    lists = K.class_index_lists_ref(lbl, img, 5)
    assert len(lists) == 5
    for c in range(5):
        assert np.array_equal(lists[c], np.nonzero(lbl[0].reshape(-1) == c)[0])
    assert sum(len(a) for a in lists) == int((lbl < 5).sum())
    mask = ((img[0] > 0.25) | (img[1] > 0.25)).reshape(-1)
    for c, a in enumerate(K.class_index_lists_ref(lbl, img, 5, image_mask=True, thr=0.25)):
        assert np.array_equal(a, np.nonzero((lbl[0].reshape(-1) == c) & mask)[0])
    multi = (rng.random((3, 5, 6, 7)) < 0.4).astype(np.int64) * 2     # any nonzero value counts; lists overlap
    lists = K.class_index_lists_ref(multi, img, None)
    for c in range(3):
        assert np.array_equal(lists[c], np.nonzero(multi[c].reshape(-1))[0])
    assert len(np.intersect1d(lists[0], lists[1])) > 0
    with pytest.raises(ValueError):
        K.class_index_lists_ref(lbl, img, None)
    with pytest.raises(ValueError):
        K.class_index_lists_ref(multi, img, 4)


def test_pick_class_rules():
    counts = [5, 5, 0, 5]
    assert K.pick_class([1, 1, 1, 1], counts, 0.0) == 0
    assert K.pick_class([1, 1, 1, 1], counts, 0.34) == 1          # total is 3: class 2 is absent
    assert K.pick_class([1, 1, 1, 1], counts, 0.67) == 3
    assert K.pick_class([0, 1, 5, 0], counts, 0.999) == 1
    assert K.pick_class([1, -1, float("nan"), float("inf")], counts, 0.999) == 0       # unchecked device values count as 0
    assert K.pick_class([0, 0, 1, 0], counts, 0.5) is None
    assert K.pick_class([0, 0, 0, 0], counts, 0.5) is None
    assert K.pick_class([1, 1, 1, 1], counts, 1.0) == 3           # past every cumulative sum: the last weighted class


def test_absent_class_is_dropped_and_other_blocks_are_pos_negs():
    shape, S = (12, 10, 9), (8, 8, 6)
    lbl = _labels(shape, 5, seed=1, absent=(2, 4))
    lists = K.class_index_lists_ref(lbl, np.zeros((1, *shape)), 5)
    assert len(lists[2]) == 0 and len(lists[4]) == 0
    cfg = _cfg(S, 64, 4, seed=9)
    tables, classes = K.replay_classes(cfg, [(shape, lists)], [1, 1, 1, 1, 1], [0], ncalls=2)
    drawn = torch.cat(classes).tolist()
    assert set(drawn) == {0, 1, 3}
    fg, bg = np.nonzero(lbl.reshape(-1))[0], np.nonzero(lbl.reshape(-1) == 0)[0]
    ref = R.replay({**cfg, "sampling": "pos_neg"}, [(shape, fg, bg)], [0], ncalls=2)
    for t, r, cl in zip(tables, ref, classes):
        assert torch.equal(t[:, 0], r[:, 0]) and torch.equal(t[:, 4:], r[:, 4:])
        for row, c in zip(t.tolist(), cl.tolist()):              # the crop holds a voxel of the class drawn
            z, y, x = row[1:4]
            assert (lbl[0, z:z + S[0], y:y + S[1], x:x + S[2]] == c).any()
    none, cl = K.replay_classes(cfg, [(shape, lists)], [0, 0, 1, 0, 1], [0], ncalls=1)
    uni = R.replay({**cfg, "sampling": "uniform"}, [(shape, fg, bg)], [0], ncalls=1)
    assert torch.equal(none[0], uni[0]) and cl[0].tolist() == [-1] * 64


def test_reference_frequencies():
    """4 calls of 256 samples on one volume, ratios [0, 1, 2, 1, 3]: every class count within 4 binomial standard deviations
    of N r_c / sum(r), class 0 never drawn.  The GPU sampler is held to this reference bit for bit and inherits the statistic."""
    shape, S = (12, 10, 9), (8, 8, 6)
    lists = K.class_index_lists_ref(_labels(shape, 5, seed=1), np.zeros((1, *shape)), 5)
    assert all(len(a) > 0 for a in lists)
    _, classes = K.replay_classes(_cfg(S, 256, 4, FREQ_SEED), [(shape, lists)], FREQ_RATIOS, [0], ncalls=4)
    drawn = torch.cat(classes)
    n, tot = drawn.numel(), sum(FREQ_RATIOS)
    assert n == 1024
    for c, r in enumerate(FREQ_RATIOS):
        p = r / tot
        got = int((drawn == c).sum())
        print(f"class {c}: drawn {got}, expected {n * p:.1f}, sd {math.sqrt(n * p * (1 - p)):.2f}")
        assert abs(got - n * p) <= 4 * math.sqrt(n * p * (1 - p)), (c, got)
    assert int((drawn == 0).sum()) == 0
