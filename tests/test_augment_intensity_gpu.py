"""GPU checks of RandCropAugment's intensity augmentation (csrc/augment.hip: aug_intensity_sample_kernel, aug_blur_*_kernel,
aug_intensity_point_kernel, aug_intensity_tone_kernel) against tests/augment_intensity_ref.py: single operations and the chain
of all five from explicit tables inside NaN red zones with a poisoned workspace, the sampler's table replayed bit for bit, the
untouched plain path, the order against normalize, graph capture, a captured TrainStep fed by it, and the argument errors.

The bounds are derived, not tuned (each test's docstring); the maxima measured on an MI355X are in profiles/intensity_augment.txt."""
import dataclasses
import math

import numpy as np
import pytest
import torch

import augment_intensity_ref as I
import augment_ref as R
from guard import Guard, poison_
from test_augment_gpu import _cache_volumes, _organs, _outputs, _volume

pytestmark = pytest.mark.gpu

B = 4
VOLUMES = [(20, 23, 19), (33, 17, 40)]
# (9, 9, 11): V = 891 is no multiple of 8 (a partial noise group) and R = 8 exceeds every extent (every tap clamps);
# (17, 17, 18): more than one AUG_BLUR_T segment along each strided axis and more than one 2048-voxel tile
CASES = [(1, 1, (12, 12, 10)), (4, 3, (16, 16, 12)), (2, 1, (9, 9, 11)), (1, 1, (17, 17, 18))]
_REF = {}       # (C, L, S, normalize) -> params, gather output x, y on the CPU: computed once, shared, never modified


def _params(S, seed):
    """[B, 8]: both volumes, corners on the borders and inside, four flip masks, every k, shift on and off"""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for r in range(B):
        dims = VOLUMES[r % 2]
        corner = [[0, dims[a] - S[a], int(torch.randint(0, dims[a] - S[a] + 1, (1,), generator=g))][(r + a) % 3] for a in range(3)]
        rows.append([r % 2, *corner, (3 * r + 1) % 8, r % 4, r % 2, I.f32_bits(0.07 if r % 2 else 0.0)])
    return torch.tensor(rows, dtype=torch.int32)


def _case(pkg, dev, C, L, S, normalize=None):
    """an augment with every probability 0 (the tables are explicit) on two volumes, its workspace poisoned, and the shared
    reference of the gather"""
    cache = pkg.VolumeCache(dev)
    for i, shape in enumerate(VOLUMES):
        cache.add(*_volume(C, L, shape, seed=60 + i, ncls=5))
    aug = pkg.RandCropAugment(cache, spatial_size=S, num_samples=4, batch_size=B, normalize=normalize, seed=9,
                              intensity=pkg.IntensityAugment())
    poison_(aug._iws.view(torch.float32))
    key = (C, L, S, normalize)
    if key not in _REF:
        images, labels = [cache.image(i)[0].cpu() for i in range(2)], [cache.label(i)[0].cpu() for i in range(2)]
        params = _params(S, seed=C + L)
        _REF[key] = (params, *R.apply_ref(images, labels, params, S, normalize=normalize is not None))
    return (aug, *_REF[key])


def _run(aug, dev, params, rows, device_table=False):
    table = torch.tensor(rows, dtype=torch.int32)
    x, y = _outputs(aug, dev)                                  # NaN everywhere: an unwritten voxel shows
    aug.apply(params, x, y, intensity=table.to(dev) if device_table else table)
    return x.cpu(), y.cpu()


def _check_rest(rows, x, y, xr, yr):
    """y and the rows without a flag are the plain gather, bit for bit"""
    assert torch.equal(y, yr)
    plain = torch.tensor([r[0] == 0 for r in rows])
    assert 0 < int(plain.sum()) < B
    assert torch.equal(x[plain], xr[plain])
    return [s for s in range(B) if rows[s][0]]


NONE = I.intensity_row()


@pytest.mark.parametrize("C,L,S", CASES)
def test_single_operations_from_explicit_tables(pkg, dev, C, L, S):
    """One operation per apply(), so its input is the gather's output, which augment_ref gives bit for bit.
    brightness: the float32 product, exactly.
    contrast:   4 * 2**-24 * max(|mn|, |mx|) from the float32 restatement with the mean from a float64 sum (equal means give
                equal bits; one ulp of the mean moves the result by at most 2 ulp).
    gamma:      2**-21 * max(rng, |mn|, |mx|) from float32 subtraction and division (correctly rounded on both sides) and a
                float64 power: powf within 2 ulp on [0, 1], one multiply, one add.
    blur:       8e-6 * max|x| from the float64 restatement: per pass the weights are within 4e-7 relative and an ordered
                float32 sum of <= 17 terms adds 17 * 2**-24; three passes give 4.2e-6, doubled.
    noise:      1e-5 * std + 2**-23 * |ref| from the float64 restatement on the same u1, u2: r <= 5.9, logf / sincosf / sqrtf
                within 2 ulp each, the float32 angle off by <= 2.4e-7: about 3.5e-6 per unit std."""
    with Guard(dev) as gd:
        aug, params, xr, yr = _case(pkg, dev, C, L, S)
        x0, y0 = _outputs(aug, dev)
        aug.apply(params, x0, y0)                               # no table: the gather alone
        assert torch.equal(x0.cpu(), xr) and torch.equal(y0.cpu(), yr)
        xn = xr.numpy()

        rows = [I.intensity_row(brightness=1.25), NONE, I.intensity_row(brightness=0.75), I.intensity_row(brightness=1.1)]
        x, y = _run(aug, dev, params, rows)
        for s in _check_rest(rows, x, y, xr, yr):
            assert torch.equal(x[s], xr[s] * torch.tensor(I.bits_f32(rows[s][5]), dtype=torch.float32))

        rows = [I.intensity_row(contrast=1.25), NONE, I.intensity_row(contrast=0.75), I.intensity_row(contrast=1.0)]
        x, y = _run(aug, dev, params, rows)
        worst = 0.0
        for s in _check_rest(rows, x, y, xr, yr):
            for c in range(C):
                mn, mx, _ = I.channel_stats(xn[s, c])
                err = float(np.abs(x[s, c].numpy().astype(np.float64) - I.contrast_f32(xn[s, c], I.bits_f32(rows[s][6]))).max())
                worst = max(worst, err / max(abs(float(mn)), abs(float(mx))))
        print(f"measured S={S} C={C}: contrast max err / max(|mn|, |mx|) = {worst:.3e} (bound {4 * 2.0 ** -24:.3e})")
        assert worst <= 4 * 2.0 ** -24

        rows = [I.intensity_row(gamma=0.7), NONE, I.intensity_row(gamma=1.5), I.intensity_row(gamma=1.0)]
        x, y = _run(aug, dev, params, rows)
        worst = 0.0
        for s in _check_rest(rows, x, y, xr, yr):
            for c in range(C):
                mn, mx, _ = I.channel_stats(xn[s, c])
                err = float(np.abs(x[s, c].numpy().astype(np.float64) - I.gamma_f64(xn[s, c], I.bits_f32(rows[s][7]))).max())
                worst = max(worst, err / max(float(mx) - float(mn), abs(float(mn)), abs(float(mx))))
        print(f"measured S={S} C={C}: gamma max err / max(rng, |mn|, |mx|) = {worst:.3e} (bound {2.0 ** -21:.3e})")
        assert worst <= 2.0 ** -21

        sig = [(0.5, 0.5, 0.5), None, (2.0, 0.5, 1.0), (1.0, 2.0, 2.0)]
        rows = [NONE if t is None else I.intensity_row(blur=t) for t in sig]
        x, y = _run(aug, dev, params, rows)
        worst = 0.0
        for s in _check_rest(rows, x, y, xr, yr):
            err = float(np.abs(x[s].numpy().astype(np.float64) - I.blur(xn[s], sig[s], np.float64)).max())
            worst = max(worst, err / float(np.abs(xn[s]).max()))
        print(f"measured S={S} C={C}: blur max err / max|x| = {worst:.3e} (bound 8e-6)")
        assert worst <= 8e-6
        x2, y2 = _run(aug, dev, params, rows, device_table=True)
        assert torch.equal(x, x2) and torch.equal(y, y2)        # a device table, and run to run the same bits

        calls = [0, None, 7, (3 << 32) | 0x80000005]            # the counter's high word reaches the Philox counter
        rows = [NONE if n is None else I.intensity_row(noise=std, call=n) for n, std in zip(calls, (0.1, 0.0, 0.05, 1.0))]
        x, y = _run(aug, dev, params, rows)
        worst = 0.0
        for s in _check_rest(rows, x, y, xr, yr):
            std = I.bits_f32(rows[s][1])
            for c in range(C):
                ref = xn[s, c].astype(np.float64) + std * I.noise_field(aug.seed, calls[s], s, c, S)
                err = np.abs(x[s, c].numpy().astype(np.float64) - ref)
                worst = max(worst, float((err / (1e-5 * std + 2.0 ** -23 * np.abs(ref))).max()))
                assert float(np.abs(x[s, c].numpy() - xn[s, c]).max()) > std          # there is noise
        print(f"measured S={S} C={C}: noise max err / (1e-5 std + 2**-23 |ref|) = {worst:.3e} (bound 1)")
        assert worst <= 1.0
    assert gd.check() > 0


def test_noise_fields_are_independent(pkg, dev):
    """channel 0 against channel 1, sample 0 against sample 1, call n against call n + 1: |correlation| < 0.05 over the 3072
    voxels of the (16, 16, 12) case (one standard error is 0.018), and each field has the moments of a unit normal"""
    C, L, S = CASES[1]
    aug, params, xr, yr = _case(pkg, dev, C, L, S)
    fields = []
    for n in (41, 42):
        x, _ = _run(aug, dev, params, [I.intensity_row(noise=1.0, call=n)] * B)
        fields.append((x - xr).numpy().astype(np.float64).reshape(B, C, -1))
    a = fields[0][0, 0]
    pairs = {"channel": fields[0][0, 1], "sample": fields[0][1, 0], "call": fields[1][0, 0]}
    for name, b in pairs.items():
        r = float(np.corrcoef(a, b)[0, 1])
        print(f"measured noise correlation across {name}: {r:+.4f}")
        assert abs(r) < 0.05, (name, r)
    z = fields[0].reshape(-1)
    assert abs(z.mean()) < 6 / math.sqrt(z.size) and abs(z.var() - 1.0) < 6 * math.sqrt(2.0 / z.size)


@pytest.mark.parametrize("C,L,S", CASES)
def test_all_five_chained(pkg, dev, C, L, S):
    """gamma in [1, 1.5] and contrast <= 1.25 (below gamma = 1 the power's slope at 0 is unbounded): within 5e-5 * scale of the
    float64 chain, scale = max|gather output| + 6 std.  The single-operation bounds sum to about 2e-5 and what follows an
    operation amplifies its error by at most 1.25 * 1.5; a skipped or misordered operation is off by 1e-2 * scale or more."""
    with Guard(dev) as gd:
        aug, params, xr, yr = _case(pkg, dev, C, L, S)
        rows = [I.intensity_row(noise=0.1, blur=(0.5, 1.0, 2.0), brightness=1.2, contrast=1.25, gamma=1.5, call=3),
                NONE,
                I.intensity_row(noise=0.05, blur=(1.0, 0.7, 0.6), brightness=0.8, contrast=0.75, gamma=1.2, call=1 << 33),
                I.intensity_row(blur=(2.0, 2.0, 2.0), contrast=1.1, gamma=1.3)]
        x, y = _run(aug, dev, params, rows)
        worst = 0.0
        for s in _check_rest(rows, x, y, xr, yr):
            scale = float(xr[s].abs().max()) + 6 * I.bits_f32(rows[s][1])
            ref = I.chain_f64(xr[s].numpy(), rows[s], aug.seed, s)
            worst = max(worst, float(np.abs(x[s].numpy().astype(np.float64) - ref).max()) / scale)
            assert float(np.abs(ref - xr[s].numpy()).max()) > 1e-2 * scale
        print(f"measured S={S} C={C}: chain max err / scale = {worst:.3e} (bound 5e-5)")
        assert worst <= 5e-5
    assert gd.check() > 0


@pytest.mark.parametrize("affine_prob", [0.0, 0.5])
def test_sampler_replays(pkg, dev, affine_prob):
    cache = pkg.VolumeCache(dev)
    for i, shape in enumerate([(20, 18, 25), (16, 30, 16), (40, 17, 19)]):
        cache.add(*_volume(1, 1, shape, seed=10 + i, ncls=3))
    kw = dict(spatial_size=(8, 8, 6), num_samples=2, batch_size=4, pos=3, neg=1, flip_prob=(0.3, 0.5, 0.7), rot90_prob=0.5, seed=4321)
    if affine_prob:
        kw.update(affine_prob=affine_prob, rotate_range=(0.5, 0.2, 0.0), zoom_range=(0.7, 1.4))
    it = pkg.IntensityAugment(noise_prob=0.5, blur_prob=0.5, brightness_prob=0.5, contrast_prob=0.5, gamma_prob=0.5)
    aug, twin = pkg.RandCropAugment(cache, intensity=it, **kw), pkg.RandCropAugment(cache, **kw)
    assert twin.intensity is None and tuple(aug.intensity.shape) == (4, 16) and aug.intensity.dtype == torch.int32
    x, y = _outputs(aug, dev)
    x2, y2 = _outputs(twin, dev)
    aug.reset(5)
    twin.reset(5)
    ref = I.replay_intensity(I.intensity_config(aug), ncalls=3, call=5)
    seen = 0
    for n in range(3):
        aug(x, y)
        twin(x2, y2)
        t = aug.intensity.cpu()
        assert torch.equal(t, ref[n]), (n, t, ref[n])
        assert torch.equal(aug.params, twin.params)
        if affine_prob:
            assert torch.equal(aug.affine, twin.affine)
        assert torch.equal(y, y2)
        plain = t[:, 0] == 0
        assert torch.equal(x.cpu()[plain], x2.cpu()[plain])
        assert bool(plain.all()) or not torch.equal(x.cpu()[~plain], x2.cpu()[~plain])
        assert bool(torch.isfinite(x).all())
        for f in t[:, 0].tolist():
            seen |= f
    assert seen == 31
    assert aug.state.cpu().tolist()[0] == 8 and twin.state.cpu().tolist()[0] == 8


@pytest.mark.parametrize("normalize", [None, "nonzero_channel_wise"])
def test_unflagged_path_is_untouched(pkg, dev, normalize):
    cache = pkg.VolumeCache(dev)
    for i, shape in enumerate([(30, 28, 26), (26, 33, 29)]):
        cache.add(*_volume(2, 3, shape, seed=20 + i))
    kw = dict(spatial_size=(16, 16, 20), num_samples=2, batch_size=4, flip_prob=(0.5, 0.5, 0.5), rot90_prob=0.5, shift_prob=0.5,
              normalize=normalize, seed=5)
    old, off = pkg.RandCropAugment(cache, **kw), pkg.RandCropAugment(cache, intensity=pkg.IntensityAugment(), **kw)
    assert old.intensity is None and old._iws is None
    (x, y), (x2, y2) = _outputs(old, dev), _outputs(off, dev)
    for _ in range(3):
        old(x, y)
        off(x2, y2)
        assert torch.equal(old.params, off.params) and torch.equal(x, x2) and torch.equal(y, y2)
        assert bool((off.intensity[:, 0] == 0).all())


def test_intensity_runs_after_normalize(pkg, dev):
    C, L, S = CASES[1]
    aug, params, xr, yr = _case(pkg, dev, C, L, S, normalize="nonzero_channel_wise")     # xr = normalize_ref(gather)
    rows = [I.intensity_row(brightness=1.2), NONE, I.intensity_row(brightness=0.8), NONE]
    x, y = _run(aug, dev, params, rows)
    assert torch.equal(y, yr)
    for s in range(B):
        assert torch.equal(x[s], xr[s] * torch.tensor(I.bits_f32(rows[s][5]), dtype=torch.float32))


def test_graph_capture_equals_eager_twin(pkg, dev):
    cache = pkg.VolumeCache(dev)
    for i, shape in enumerate([(30, 28, 26), (26, 33, 29)]):
        cache.add(*_volume(2, 3, shape, seed=20 + i))
    it = dataclasses.replace(pkg.IntensityAugment.nnunet(), noise_prob=0.5, blur_prob=0.5, brightness_prob=0.5, contrast_prob=0.5,
                             gamma_prob=0.5)
    kw = dict(spatial_size=16, num_samples=2, batch_size=4, flip_prob=(0.5, 0.5, 0.5), rot90_prob=0.5, shift_prob=0.5,
              normalize="nonzero_channel_wise", seed=5, intensity=it)
    aug, twin = pkg.RandCropAugment(cache, **kw), pkg.RandCropAugment(cache, **kw)
    x, y = _outputs(aug, dev)
    x2, y2 = _outputs(twin, dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        aug(x, y)                                              # no synchronising call inside
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        aug(x, y)
    aug.reset(0)
    twin.reset(0)
    seen, first = 0, []
    for _ in range(3):
        graph.replay()
        twin(x2, y2)
        torch.cuda.synchronize()
        assert torch.equal(aug.params, twin.params) and torch.equal(aug.intensity, twin.intensity)
        assert torch.equal(x, x2) and torch.equal(y, y2)
        first.append((x2.clone(), twin.intensity.clone()))
        for f in aug.intensity[:, 0].tolist():
            seen |= f
    assert seen == 31 and aug.state.cpu().tolist()[0] == 3
    twin.reset(0)
    for xa, ta in first:                                       # the eager twin again from reset(): identical bits
        twin(x2, y2)
        assert torch.equal(x2, xa) and torch.equal(twin.intensity, ta)


def test_feeds_captured_train_step_without_host_sync(pkg, dev):
    C1 = dict(in_channels=1, out_channels=2, img_size=(32, 32, 32), feature_size=16, hidden_size=128, mlp_dim=512,
              num_heads=4, pos_embed="perceptron", norm_name="instance", res_block=True)
    cache = pkg.VolumeCache(dev)
    img, lbl = _organs(1, 1, (64, 60, 48), 2, seed=3)
    cache.add(img, lbl, scale_range=(-175, 250, 0.0, 1.0), crop_foreground=True)
    aug = pkg.RandCropAugment(cache, spatial_size=32, num_samples=2, pos=1, neg=1, seed=0, intensity=pkg.IntensityAugment.nnunet())
    x = torch.empty(2, 1, 32, 32, 32, device=dev)
    y = torch.empty(2, 1, 32, 32, 32, device=dev)
    aug(x, y)
    torch.manual_seed(0)
    m = pkg.UNETRLogits(**C1).to(dev)
    m.precision = "bf16"
    flat = m.use_flat_buffers()
    opt = pkg.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-5, flat=flat)
    step = pkg.TrainStep(m, pkg.DiceCELoss(to_onehot_y=True, softmax=True), opt, x, y, use_graph=True, warmup=2)
    assert step.graphs is not None
    prev = x.clone()
    for _ in range(3):
        torch.cuda.set_sync_debug_mode("error")
        try:
            aug(x, y)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        step.run()
        torch.cuda.synchronize()
        assert not torch.equal(x, prev) and bool(torch.isfinite(x).all())
        prev = x.clone()
        assert math.isfinite(float(step.loss.detach()))


def test_apply_table_errors(pkg, dev):
    cache = pkg.VolumeCache(dev)
    cache.add(*_volume(1, 1, (12, 12, 12), seed=1))
    mk = lambda **kw: pkg.RandCropAugment(cache, spatial_size=8, num_samples=2, **kw)  # noqa: E731
    plain, aug = mk(), mk(intensity=pkg.IntensityAugment())
    x, y = _outputs(aug, dev)
    params = torch.zeros(2, 8, dtype=torch.int32)
    good = torch.tensor([NONE, I.intensity_row(noise=0.1, blur=(0.5, 2.0, 1.0), brightness=1.1, contrast=0.9, gamma=0.7)],
                        dtype=torch.int32)
    aug.apply(params, x, y, intensity=good)
    assert not bool(torch.isnan(x).any())
    aug.apply(params, x, y)                                    # no table: no operation is flagged
    with pytest.raises(ValueError, match="built with intensity"):
        plain.apply(params, x, y, intensity=good)
    with pytest.raises(ValueError, match=r"intensity \[2, 16\]"):
        aug.apply(params, x, y, intensity=good[:, :12])
    nan, inf = float("nan"), float("inf")
    for col, val, msg in ((0, 32, "flag bits"), (0, -1, "flag bits"), (3, I.f32_bits(2.5), "sigma"), (2, I.f32_bits(0.0), "sigma"),
                          (1, I.f32_bits(nan), "finite"), (5, I.f32_bits(inf), "finite"), (1, I.f32_bits(-0.1), "noise std"),
                          (6, I.f32_bits(0.0), "positive"), (7, I.f32_bits(-1.0), "positive")):
        bad = good.clone()
        bad[1, col] = val
        with pytest.raises(ValueError, match=msg):
            aug.apply(params, x, y, intensity=bad)
