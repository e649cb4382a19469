"""Host side of mirror test-time augmentation and ensembling in SlidingWindowInferer (no GPU): the expanded window table, the
parsing of ``tta_flips``, argument checking, and the float64 reference's own algebra."""
import pytest
import torch

from inference_ref import ref_sliding_window
from tta_ref import flip, ref_tta_sliding_window

ROI = (32, 32, 32)
# (volume, batch, overlap, sw_batch_size): full rows only | a tail row | one window per item
PLANS = [((48, 48, 48), 2, 0.25, 4), ((48, 48, 48), 1, 0.25, 3), ((32, 32, 32), 2, 0.25, 4)]


@pytest.mark.parametrize("size,batch,overlap,n", PLANS)
def test_plan_without_flips_is_the_old_table(pkg, size, batch, overlap, n):
    old_t, old_c = pkg.inference.plan_window_table(batch, size, ROI, overlap, n)
    new_t, new_c = pkg.inference.plan_window_table(batch, size, ROI, overlap, n, flips=None)
    assert new_t.dtype == old_t.dtype and torch.equal(new_t, old_t) and new_c == old_c
    assert bool((old_t[:, 1:4] == 0).all())


@pytest.mark.parametrize("size,batch,overlap,n", PLANS)
def test_plan_with_flips_repeats_every_row_per_flip(pkg, size, batch, overlap, n):
    flips = [0, 5, 2]
    old_t, old_c = pkg.inference.plan_window_table(batch, size, ROI, overlap, n)
    new_t, new_c = pkg.inference.plan_window_table(batch, size, ROI, overlap, n, flips=flips)
    assert new_t.dtype == torch.int32 and tuple(new_t.shape) == (3 * old_t.shape[0], pkg._capi.SW_ROW_INTS)
    assert new_c == [c for c in old_c for _ in flips]
    for r in range(old_t.shape[0]):
        for k, f in enumerate(flips):
            row = new_t[3 * r + k]
            assert int(row[1]) == f and int(row[0]) == old_c[r] and row[2:4].tolist() == [0, 0]
            assert torch.equal(row[4:], old_t[r, 4:])
    # an inferer plans with its own flips
    inferer = pkg.SlidingWindowInferer(ROI, n, overlap=overlap, tta_flips=[(), (0, 2), (1,)])
    t, c = inferer._plan(batch, size, ROI)
    assert torch.equal(t, new_t) and c == new_c
    t, c = pkg.SlidingWindowInferer(ROI, n, overlap=overlap)._plan(batch, size, ROI)
    assert torch.equal(t, old_t) and c == old_c


def test_tta_flips_forms(pkg):
    fm = pkg.inference.flip_masks
    assert fm(None) is None
    assert fm("all") == list(range(8))
    assert fm([(), (0,), (1, 2)]) == [0, 1, 6]
    assert fm([(2, 0), 3, (1,)]) == [5, 3, 2]          # given order kept; bit a = spatial axis a
    assert fm(((0, 1, 2),)) == [7]
    assert pkg.SlidingWindowInferer(ROI, 4, tta_flips="all").tta_flips == list(range(8))
    assert pkg.SlidingWindowInferer(ROI, 4).tta_flips is None and pkg.SlidingWindowInferer(ROI, 4).activation is None


@pytest.mark.parametrize("bad", [[], (), [(3,)], [(-1,)], [(0, 0)], [8], [-1], [(0,), 1], [(0, 1), (1, 0)], [0, 0], "none", 3, [1.0],
                                 [(0.0,)], ["all"], [None]])
def test_bad_tta_flips_are_rejected(pkg, bad):
    with pytest.raises(ValueError):
        pkg.SlidingWindowInferer(ROI, 4, tta_flips=bad)


def test_bad_activation_is_rejected(pkg):
    with pytest.raises(ValueError):
        pkg.SlidingWindowInferer(ROI, 4, activation="tanh")
    for act in (None, "softmax", "sigmoid"):
        assert pkg.SlidingWindowInferer(ROI, 4, activation=act).activation == act


def test_post_and_activation_combinations(pkg):
    """post="sigmoid" cannot follow activation="softmax" (ValueError before anything runs); every other combination gets past the
    argument checks -- on a CPU tensor that is the "no CPU fallback" error"""
    x = torch.zeros(1, 1, 32, 32, 32)
    net = lambda w: w
    with pytest.raises(ValueError, match="softmax"):
        pkg.SlidingWindowInferer(ROI, 4, activation="softmax")(x, net, post="sigmoid")
    with pytest.raises(ValueError):
        pkg.SlidingWindowInferer(ROI, 4, activation="sigmoid")(x, net, post="threshold")
    with pytest.raises(ValueError):
        pkg.SlidingWindowInferer(ROI, 4)(x, [])                                  # an empty ensemble
    for act, posts in ((None, (None, "onehot", "argmax", "sigmoid")), ("sigmoid", (None, "onehot", "argmax", "sigmoid")),
                       ("softmax", (None, "onehot", "argmax"))):
        for post in posts:
            with pytest.raises(RuntimeError, match="ROCm device"):
                pkg.SlidingWindowInferer(ROI, 4, activation=act, tta_flips="all")(x, [net, net], post=post)
    thr = pkg.inference._finalize_threshold
    assert thr("sigmoid", None) == 0.0 and thr("sigmoid", "sigmoid") == 0.5


def test_reference_identities():
    """the float64 reference: flip mask 0 and one model is plain blending; a flip-equivariant predictor is unchanged by any set of
    flips; bit a of a mask reverses spatial axis a"""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 1, 20, 24, 36, generator=g, dtype=torch.float64)
    roi = (16, 16, 16)
    imp = torch.rand(*roi, generator=g, dtype=torch.float64) + 0.05
    pointwise = lambda w: torch.cat([w * 2.0 + 1.0, w * w], 1)
    plain = ref_sliding_window(x, roi, 3, pointwise, overlap=0.5, importance=imp)
    assert torch.equal(ref_tta_sliding_window(x, roi, 3, [pointwise], [0], overlap=0.5, importance=imp), plain)
    both = ref_tta_sliding_window(x, roi, 3, [pointwise, pointwise], list(range(8)), overlap=0.5, importance=imp)
    assert (both - plain).abs().max().item() < 1e-12
    ramp = torch.arange(16, dtype=torch.float64)[None, None, None, None, :]      # not flip-equivariant along x
    skew = lambda w: w * ramp
    a = ref_tta_sliding_window(x, roi, 3, [skew], [0, 4], overlap=0.5, importance=imp)
    assert (a - ref_sliding_window(x, roi, 3, lambda w: w * 7.5, overlap=0.5, importance=imp)).abs().max().item() < 1e-12
    t = torch.arange(2 * 3 * 4).reshape(1, 1, 2, 3, 4)
    assert torch.equal(flip(t, 1), t.flip(2)) and torch.equal(flip(t, 4), t.flip(4)) and torch.equal(flip(t, 6), t.flip(3, 4))
