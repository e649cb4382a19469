"""CPU checks of the augmentation restatements (tests/augment_ref.py) and of RandCropAugment's argument checks: the Philox
restatement against numpy.random.Philox, correct_crop_centers, the composed index map against sequential flips / rot90."""
import numpy as np
import pytest
import torch

import augment_ref as R


@pytest.mark.parametrize("key,counter", [((0, 0), (0, 0, 0, 0)), ((1, 2), (0, 0, 0, 0)), ((3, 0), (4, 7, 9, 0)),
                                         ((2 ** 64 - 1, 5), (2 ** 64 - 3, 1, 2 ** 63, 3))])
def test_philox_matches_numpy(key, counter):
    """numpy's first block is philox4x64_10(counter + 1): numpy increments its 256-bit counter before every block"""
    ref = np.random.Philox(key=np.array(key, dtype=np.uint64), counter=np.array(counter, dtype=np.uint64)).random_raw(8).tolist()
    c1 = list(counter)
    c1[0] = (c1[0] + 1) & R.M64
    c2 = list(c1)
    c2[0] = (c2[0] + 1) & R.M64
    assert R.philox4x64_10(c1, key) + R.philox4x64_10(c2, key) == ref


def test_philox_counter_carry_matches_numpy():
    ref = np.random.Philox(key=np.array([9, 9], dtype=np.uint64),
                           counter=np.array([R.M64, 4, 0, 0], dtype=np.uint64)).random_raw(4).tolist()
    assert R.philox4x64_10((0, 5, 0, 0), (9, 9)) == ref


def test_draw_conventions():
    assert R.u01(0) == 0.0 and R.u01(R.M64) == 1.0 - 2.0 ** -53
    assert R.randint(0, 7) == 0 and R.randint(R.M64, 7) == 6
    # numpy's Generator(Philox).random() is the same (w >> 11) * 2**-53 of the next raw word
    g = np.random.Generator(np.random.Philox(key=[5, 0], counter=[0, 0, 0, 0]))
    w = R.philox4x64_10((1, 0, 0, 0), (5, 0))
    assert [g.random() for _ in range(4)] == [R.u01(x) for x in w]


@pytest.mark.parametrize("S", [4, 5, 96, 97])
def test_correct_crop_centers_table(S):
    for dim in (S, S + 1, S + 7, 3 * S + 2):
        for c in (0, S // 2 - 1, S // 2, dim // 2, dim - S // 2 - 1, dim - S // 2, dim - 1):
            c = max(0, min(dim - 1, c))
            (cc,) = R.correct_crop_centers([c], [S], [dim])
            z0 = R.crop_corner([cc], [S])[0]
            assert 0 <= z0 and z0 + S <= dim, (S, dim, c, cc)
            if S // 2 <= c and c - S // 2 + S <= dim:
                assert cc == c               # a centre whose crop fits is kept
    # dim == S: the only crop is the whole axis
    assert R.correct_crop_centers([0, 5, 9], [10, 10, 10], [10, 10, 10]) == [5, 5, 5]
    assert R.correct_crop_centers([0, 2, 4], [5, 5, 5], [5, 5, 5]) == [2, 2, 2]
    # valid_end = floor(dim + 1 - S / 2): S = 5, dim = 8 -> centres 2..5
    assert R.correct_crop_centers([0, 7, 4], [5, 5, 5], [8, 8, 8]) == [2, 5, 4]


@pytest.mark.parametrize("axes", [(0, 1), (1, 2), (0, 2)])
def test_composed_index_matches_sequential_flip_rot90(axes):
    g = torch.Generator().manual_seed(0)
    for flips in range(8):
        for k in range(4):
            S = [5, 5, 5]
            free = 3 - axes[0] - axes[1]
            S[free] = 3 + flips % 3                          # non-cubic along the axis the rotation leaves alone
            S = tuple(S)
            vol = torch.randn(2, 9, 8, 10, generator=g)
            corner = [int(torch.randint(0, d - s + 1, (1,), generator=g)) for d, s in zip(vol.shape[1:], S)]
            seq = R.augment_seq(vol, corner, S, flips, k, axes)
            idx = R.source_index(S, corner, flips, k, axes)
            gat = vol[:, idx[0], idx[1], idx[2]]
            assert torch.equal(seq, gat), (flips, k, axes)


class _Shapes:
    """a stand-in cache: RandCropAugment validates its arguments against cache.shapes before touching a device"""
    device = torch.device("cpu")

    def __init__(self, *shapes):
        self.shapes = list(shapes)


@pytest.mark.parametrize("kw,match", [
    (dict(spatial_size=(8, 6, 8)), "equal crop sizes"),
    (dict(spatial_size=(8, 8, 6), spatial_axes=(1, 2)), "equal crop sizes"),
    (dict(num_samples=4, batch_size=6), "multiple of num_samples"),
    (dict(pos=0, neg=0), "pos=0 and neg=0"),
    (dict(spatial_size=40), "smaller than the crop"),
    (dict(spatial_size=(8, 8, 33)), "smaller than the crop"),
    (dict(normalize="nonzero"), "normalize must be one of"),
    (dict(sampling="weighted"), "sampling must be one of"),
    (dict(spatial_axes=(1, 1)), "spatial_axes"),
    (dict(max_k=0), "max_k"),
])
def test_constructor_errors(pkg, kw, match):
    with pytest.raises(ValueError, match=match):
        pkg.RandCropAugment(_Shapes((1, 1, 40, 36, 32)), **{"spatial_size": 8, **kw})


def test_constructor_mixed_channels_and_empty_cache(pkg):
    with pytest.raises(ValueError, match="label channels"):
        pkg.RandCropAugment(_Shapes((1, 1, 16, 16, 16), (4, 3, 16, 16, 16)), spatial_size=8)
    with pytest.raises(ValueError, match="no volume"):
        pkg.RandCropAugment(_Shapes(), spatial_size=8)


def test_volume_cache_needs_a_gpu_device(pkg):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.VolumeCache("cpu")


def test_replay_is_deterministic_and_in_range():
    cfg = dict(spatial_size=(4, 4, 4), sampling="pos_neg", pos_ratio=0.5, flip_prob=(0.5, 0.5, 0.5), rot90_prob=0.5, max_k=3,
               shift_prob=0.5, shift_range=(-0.1, 0.1), num_samples=2, batch_size=4, seed=3)
    shape = (9, 7, 6)
    fg, bg = [0, 17, 377], list(range(1, 300, 7))
    a = R.replay(cfg, [(shape, fg, bg)], [0], ncalls=5)
    b = R.replay(cfg, [(shape, fg, bg)], [0], ncalls=5)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    t = torch.stack(a)
    for ax in range(3):
        assert int(t[..., 1 + ax].min()) >= 0 and int(t[..., 1 + ax].max()) <= shape[ax] - 4
    assert set(t[..., 5].unique().tolist()) <= {0, 1, 2, 3}
