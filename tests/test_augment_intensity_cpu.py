"""CPU checks of the intensity augmentation: IntensityAugment's validation, the exports and the C ABI's new symbols, and the
anchors of tests/augment_intensity_ref.py, the restatement the GPU tests pin csrc/augment.hip's intensity kernels to."""
import math
import os
import re

import numpy as np
import pytest
import torch

import augment_intensity_ref as I
import augment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("unetr_aug_intensity_sample", "unetr_aug_intensity_ws_bytes", "unetr_aug_intensity_apply")


# ---------------------------------------------------------------- the public dataclass
def test_defaults_and_nnunet(pkg):
    it = pkg.IntensityAugment()
    assert (it.noise_prob, it.blur_prob, it.brightness_prob, it.contrast_prob, it.gamma_prob) == (0.0,) * 5
    assert it.noise_std == (0.0, 0.1) and it.blur_sigma == (0.5, 1.0) and it.brightness_range == (0.75, 1.25)
    assert it.contrast_range == (0.75, 1.25) and it.gamma_range == (0.7, 1.5)
    nn = pkg.IntensityAugment.nnunet()
    assert (nn.noise_prob, nn.blur_prob, nn.brightness_prob, nn.contrast_prob, nn.gamma_prob) == (0.1, 0.2, 0.15, 0.15, 0.3)
    assert (nn.noise_std, nn.blur_sigma, nn.brightness_range, nn.contrast_range, nn.gamma_range) == \
        (it.noise_std, it.blur_sigma, it.brightness_range, it.contrast_range, it.gamma_range)
    with pytest.raises(Exception):                              # frozen
        it.noise_prob = 0.5
    assert pkg.IntensityAugment(blur_sigma=[1, 2]).blur_sigma == (1.0, 2.0)


@pytest.mark.parametrize("name", ["noise_prob", "blur_prob", "brightness_prob", "contrast_prob", "gamma_prob"])
def test_probabilities_lie_in_0_1(pkg, name):
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=name):
            pkg.IntensityAugment(**{name: bad})
    assert getattr(pkg.IntensityAugment(**{name: 1}), name) == 1.0


@pytest.mark.parametrize("name", ["noise_std", "blur_sigma", "brightness_range", "contrast_range", "gamma_range"])
def test_ranges_are_finite_and_ordered(pkg, name):
    for bad in ((1.0, 0.5), (0.5, float("inf")), (float("nan"), 1.0), (1.0,), 0.5):
        with pytest.raises(ValueError, match=name):
            pkg.IntensityAugment(**{name: bad})


def test_range_limits(pkg):
    with pytest.raises(ValueError, match="noise_std"):
        pkg.IntensityAugment(noise_std=(-0.1, 0.1))
    assert pkg.IntensityAugment(noise_std=(0.0, 0.0)).noise_std == (0.0, 0.0)
    for bad in ((0.0, 1.0), (-1.0, 1.0), (0.5, 2.5)):
        with pytest.raises(ValueError, match="blur_sigma"):
            pkg.IntensityAugment(blur_sigma=bad)
    assert pkg.IntensityAugment(blur_sigma=(2.0, 2.0)).blur_sigma == (2.0, 2.0)
    for name in ("brightness_range", "contrast_range", "gamma_range"):
        for bad in ((0.0, 1.0), (-0.5, 1.0)):
            with pytest.raises(ValueError, match=name):
                pkg.IntensityAugment(**{name: bad})


def test_construction_errors_before_any_device_work(pkg):
    """what RandCropAugment raises before it touches a device: a stub cache is enough, as for the affine arguments"""
    class Stub:
        shapes = [(1, 1, 12, 12, 12)]
    with pytest.raises(ValueError, match="IntensityAugment"):
        pkg.RandCropAugment(Stub(), spatial_size=8, num_samples=2, intensity=dict(noise_prob=0.5))
    with pytest.raises(ValueError, match="IntensityAugment"):
        pkg.RandCropAugment(Stub(), spatial_size=8, num_samples=2, intensity=0.5)


def test_exports_and_abi(pkg):
    assert "IntensityAugment" in pkg.__all__ and pkg.IntensityAugment is pkg.augment.IntensityAugment
    assert pkg._capi.ABI_VERSION == 21
    header = open(os.path.join(ROOT, "include", "unetr_hip.h")).read()
    assert int(re.search(r"#define\s+UNETR_ABI_VERSION\s+(\d+)", header).group(1)) == 21
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for s in NEW_SYMBOLS:
        assert s in pkg._capi.EXPORTED_SYMBOLS, s
        assert re.search(r"\b%s\s*\(" % s, code), s
    assert "UnetrAugIntensityDesc" in code
    d = pkg.IntensityAugment.nnunet()._desc()
    assert list(d.prob) == [0.1, 0.2, 0.15, 0.15, 0.3] and list(d.lo) == [0.0, 0.5, 0.75, 0.75, 0.7]
    assert list(d.hi) == [0.1, 1.0, 1.25, 1.25, 1.5]


# ---------------------------------------------------------------- the reference checks itself
def test_replay_uses_blocks_5_to_7_and_neutral_values():
    cfg = dict(noise_prob=0.5, noise_std=(0.0, 0.1), blur_prob=0.5, blur_sigma=(0.5, 1.0), brightness_prob=0.5,
               brightness_range=(0.75, 1.25), contrast_prob=0.5, contrast_range=(0.75, 1.25), gamma_prob=0.5,
               gamma_range=(0.7, 1.5), batch_size=8, seed=77)
    a, b = I.replay_intensity(cfg, 3), I.replay_intensity(cfg, 3)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(I.replay_intensity(cfg, 1, call=2)[0], a[2])
    seen = 0
    for n, t in enumerate(a):
        for s, row in enumerate(t.tolist()):
            flags, std, sg, br, ct, gm, call = I.row_values(row)
            assert call == n and row[10:] == [0] * 6 and 0 <= flags <= 31
            seen |= flags
            assert (0.0 <= std <= 0.1) if flags & I.NOISE else std == 0.0
            assert all(0.5 <= v <= 1.0 for v in sg) if flags & I.BLUR else sg == (0.0, 0.0, 0.0)
            assert (0.75 <= br <= 1.25) if flags & I.BRIGHTNESS else br == 1.0
            assert (0.75 <= ct <= 1.25) if flags & I.CONTRAST else ct == 1.0
            assert (0.7 <= gm <= 1.5) if flags & I.GAMMA else gm == 1.0
            w = I.intensity_words(77, n, s)
            assert w == [R.philox4x64_10((n, s, j, 0), (77, 0)) for j in (5, 6, 7)]
            assert all(blk not in R.sample_words(77, n, s) for blk in w)
    assert seen == 31
    big = I.intensity_row(noise=0.1, call=(5 << 32) | 0x80000001)
    assert I.row_values(big)[6] == (5 << 32) | 0x80000001 and all(-2 ** 31 <= v < 2 ** 31 for v in big)


def test_vector_philox_equals_the_scalar_one():
    g = np.arange(50, dtype=np.uint64) + np.uint64(2 ** 33 - 20)
    got = I.philox4x64_10_np((3, 7, 18, g), (2 ** 63 + 5, 0))
    for i, gi in enumerate(g.tolist()):
        assert [int(w[i]) for w in got] == R.philox4x64_10((3, 7, 18, gi), (2 ** 63 + 5, 0))


@pytest.mark.parametrize("sigma,radius", [(0.5, 2), (1.0, 4), (2.0, 8)])
def test_blur_weights_sum_to_one_and_keep_a_constant(sigma, radius):
    assert I.blur_radius(sigma) == radius
    w = I.blur_weights(sigma)
    assert w.dtype == np.float32 and len(w) == 2 * radius + 1 and np.array_equal(w, w[::-1])
    assert abs(float(w.astype(np.float64).sum()) - 1.0) <= 2.0 ** -22
    const = np.full((2, 5, 9, 7), 3.7, dtype=np.float32)          # extents below the radius: every tap clamps
    out = I.blur(const, (sigma, sigma, sigma))
    assert out.dtype == np.float32 and float(np.abs(out / np.float32(3.7) - 1.0).max()) <= 2.0 ** -22


def test_blur_is_border_padded_and_separable():
    g = np.random.default_rng(0)
    x = g.standard_normal((1, 6, 7, 20)).astype(np.float32)
    out = I.blur(x, (0.5, 1.0, 2.0), np.float64)
    want = x.astype(np.float64)
    for a, sg in enumerate((0.5, 1.0, 2.0)):
        w = I.blur_weights(sg, np.float64)
        rad = len(w) // 2
        pad = [(0, 0)] * 4
        pad[1 + a] = (rad, rad)
        p = np.pad(want, pad, mode="edge")
        want = sum(w[k] * np.take(p, np.arange(want.shape[1 + a]) + k, axis=1 + a) for k in range(2 * rad + 1))
    assert float(np.abs(out - want).max()) <= 1e-14


def test_box_muller_moments():
    """2**16 groups of 8 normals: |mean| < 6 / sqrt(N), |var - 1| < 6 sqrt(2 / N) (six standard errors)"""
    N = 8 * 2 ** 16
    for dtype in (np.float64, np.float32):
        z = I.noise_field(1234, 3, 1, 2, (N,), dtype).astype(np.float64)
        assert z.shape == (N,) and bool(np.isfinite(z).all())
        assert abs(z.mean()) < 6 / math.sqrt(N) and abs(z.var() - 1.0) < 6 * math.sqrt(2.0 / N)
    u1, u2 = I.noise_uniforms(1234, 3, 1, 2, 2 ** 16)
    assert u1.dtype == np.float32 and float(u1.min()) > 0.0 and float(u1.max()) <= 1.0 and float(u2.min()) > 0.0
    # a partial group takes the first normals; channel, sample and call key different fields
    a = I.noise_field(5, 0, 0, 0, (9, 9, 11))
    assert np.array_equal(a.reshape(-1), I.noise_field(5, 0, 0, 0, (896,)).reshape(-1)[:891])
    for other in (I.noise_field(5, 0, 0, 1, (9, 9, 11)), I.noise_field(5, 0, 1, 0, (9, 9, 11)), I.noise_field(5, 1, 0, 0, (9, 9, 11))):
        assert abs(np.corrcoef(a.reshape(-1), other.reshape(-1))[0, 1]) < 0.2


def test_neutral_contrast_and_gamma_return_their_input():
    g = np.random.default_rng(1)
    for scale, shift in ((1.0, 0.0), (50.0, -120.0), (1e-3, 4.0)):
        x = (g.standard_normal((12, 10, 9)) * scale + shift).astype(np.float32)
        ulp = 2.0 ** -23 * max(abs(float(x.min())), abs(float(x.max())))
        assert float(np.abs(I.contrast_f32(x, 1.0).astype(np.float64) - x).max()) <= 2 * ulp
        assert float(np.abs(I.gamma_f32(x, 1.0).astype(np.float64) - x).max()) <= 2 * ulp
        assert float(np.abs(I.gamma_f64(x, 1.0) - x).max()) <= 2 * ulp
    x = g.standard_normal((6, 6, 6)).astype(np.float32)
    c = I.contrast_f32(x, 1.25)
    assert float(c.min()) >= float(x.min()) and float(c.max()) <= float(x.max()) and float(c.std()) > float(x.std())
    gm = I.gamma_f32(x, 1.5)
    assert abs(float(gm.min()) - float(x.min())) <= 1e-6 and abs(float(gm.max()) - float(x.max())) <= 1e-6
    assert float(gm.mean()) < float(x.mean())                   # gamma > 1 darkens
