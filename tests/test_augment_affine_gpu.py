"""GPU checks of RandCropAugment's random rotation and zoom (csrc/augment.hip: aug_sample_kernel<true>, aug_gather_kernel<., true>)
against tests/augment_affine_ref.py, bit for bit: explicit tables inside NaN red zones, the sampler's affine table replayed, the
untouched plain path, a shrunk CT configuration end to end, graph capture and the argument errors."""
import struct

import numpy as np
import pytest
import torch

import augment_affine_ref as A
import augment_ref as R
from guard import Guard
from test_augment_gpu import _cache_volumes, _organs, _outputs, _volume

pytestmark = pytest.mark.gpu

NORMALIZE = (None, "nonzero_channel_wise")


def _quarter_turn(axis, sign):
    a, b = (axis + 1) % 3, (axis + 2) % 3
    m = np.zeros((3, 3))
    m[axis, axis] = 1.0
    m[a, b], m[b, a] = -sign, sign
    return m


def _affine_kinds():
    """the eight kinds of rows an explicit table mixes"""
    return [A.IDENTITY_ROW,                                                            # unflagged
            A.affine_row(matrix=_quarter_turn(0, 1.0)), A.affine_row(matrix=_quarter_turn(1, -1.0)),
            A.affine_row(matrix=_quarter_turn(2, 1.0) @ np.diag([1.0, -1.0, 1.0])),    # exact signed permutations
            A.affine_row(zooms=(0.5, 0.5, 0.5)), A.affine_row(zooms=(2.0, 2.0, 2.0)),  # pure zoom, exact in binary
            A.affine_row(angles=(0.3, -0.2, 0.5), zooms=(1.25, 0.8, 1.1)),             # generic rotation, anisotropic zoom
            A.affine_row(angles=(-0.7, 0.4, -1.1), zooms=(0.6, 1.5, 0.9))]


def _tables(shapes, S, B, seed):
    """params [B, 8] and affine [B, 16]: every k with four flip masks, corners on the borders and inside, shift on and off, the
    kinds of _affine_kinds shifted against k from one half of the table to the other"""
    g = torch.Generator().manual_seed(seed)
    kinds = _affine_kinds()
    rows, arows = [], []
    for r in range(B):
        vol = r % len(shapes)
        dims = shapes[vol]
        corner = []
        for a in range(3):
            hi = dims[a] - S[a]
            corner.append([0, hi, int(torch.randint(0, hi + 1, (1,), generator=g))][(r + a) % 3])
        flips, k, shift = (3 * r + r // 4) % 8, r % 4, r % 2
        off = float(torch.rand(1, generator=g)) * 0.2 - 0.1 if shift else 0.0
        rows.append([vol, *corner, flips, k, shift, struct.unpack("<i", struct.pack("<f", off))[0]])
        arows.append(kinds[(r + r // 8) % 8])
    return torch.tensor(rows, dtype=torch.int32), torch.tensor(arows, dtype=torch.float32)


# (17, 17, 18) is not in the issue's list: it is the smallest crop that is cut into more than one brick along every axis
@pytest.mark.parametrize("C,L,S", [(1, 1, (12, 12, 10)), (4, 3, (16, 16, 12)), (2, 1, (9, 9, 11)), (1, 1, (17, 17, 18))])
def test_apply_explicit_affine_tables(pkg, dev, C, L, S):
    B = 16
    with Guard(dev) as gd:
        cache = pkg.VolumeCache(dev)
        for i, shape in enumerate([(20, 23, 19), (33, 17, 40), S]):      # the last: every side of a warped footprint clamps
            cache.add(*_volume(C, L, shape, seed=40 + i, ncls=14))
        images = [cache.image(i)[0].cpu() for i in range(3)]
        labels = [cache.label(i)[0].cpu() for i in range(3)]
        table, atab = _tables([s[2:] for s in cache.shapes], S, B, seed=C + L)
        plain = atab[:, 0] == 0
        assert 0 < int(plain.sum()) < B
        for normalize in NORMALIZE:
            aug = pkg.RandCropAugment(cache, spatial_size=S, num_samples=4, batch_size=B, normalize=normalize, affine_prob=1.0,
                                      rotate_range=0.1)
            x, y = _outputs(aug, dev)                              # NaN everywhere: an unwritten voxel shows
            aug.apply(table, x, y, affine=atab)
            xr, yr = A.apply_affine_ref(images, labels, table, atab, S, normalize=normalize is not None)
            xc, yc = x.cpu(), y.cpu()
            print(f"S={S} normalize={normalize}: max |x - ref| = {float((xc - xr).abs().max()):.3e}, "
                  f"voxels differing: {int((xc != xr).sum())} of {xr.numel()}, y: {int((yc != yr).sum())}")
            assert torch.equal(yc, yr)
            assert torch.equal(xc, xr)
            x0, y0 = R.apply_ref(images, labels, table[plain], S, normalize=normalize is not None)
            assert torch.equal(xc[plain], x0) and torch.equal(yc[plain], y0)      # unflagged rows: the plain gather, exactly
            x2, y2 = _outputs(aug, dev)
            aug.apply(table.to(dev), x2, y2, affine=atab.to(dev))
            assert torch.equal(x, x2) and torch.equal(y, y2)       # device tables, run to run bit-identical
    assert gd.check() > 0


@pytest.mark.parametrize("per_axis", [False, True])
def test_affine_sampler_replays(pkg, dev, per_axis):
    cache = pkg.VolumeCache(dev)
    for i, shape in enumerate([(20, 18, 25), (16, 30, 16), (40, 17, 19)]):
        cache.add(*_volume(1, 1, shape, seed=10 + i, ncls=3))
    aug = pkg.RandCropAugment(cache, spatial_size=(8, 8, 6), num_samples=4, batch_size=8, pos=3, neg=1, flip_prob=(0.3, 0.5, 0.7),
                              rot90_prob=0.5, seed=4321, affine_prob=0.5, rotate_range=(0.5, 0.2, 0.0), zoom_range=(0.7, 1.4),
                              zoom_per_axis=per_axis)
    images, labels = [cache.image(i)[0].cpu() for i in range(3)], [cache.label(i)[0].cpu() for i in range(3)]
    x, y = _outputs(aug, dev)
    order = [2, 0, 1]
    aug.set_order(order)
    cfg = A.affine_config(aug)
    ref_p = R.replay(cfg, _cache_volumes(cache), order, ncalls=4)
    ref_a = A.replay_affine(cfg, ncalls=4)
    flagged = 0
    for n in range(4):
        aug(x, y)
        p, a = aug.params.cpu(), aug.affine.cpu()
        assert torch.equal(p, ref_p[n])
        assert torch.equal(a[:, :7].contiguous().view(torch.int32), ref_a[n][:, :7].contiguous().view(torch.int32)), (n, a, ref_a[n])
        want = ref_a[n][:, 7:].numpy()
        assert np.all(np.abs(a[:, 7:].numpy().astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))), (n, a, ref_a[n])
        xr, yr = A.apply_affine_ref(images, labels, p, a, aug.spatial_size)          # the reference fed the device's matrix
        assert torch.equal(x.cpu(), xr) and torch.equal(y.cpu(), yr)
        flagged += int(a[:, 0].sum())
    assert 0 < flagged < 32
    assert aug.state.cpu().tolist()[0] == 4


@pytest.mark.parametrize("normalize", NORMALIZE)
def test_plain_path_is_untouched(pkg, dev, normalize):
    cache = pkg.VolumeCache(dev)
    for i, shape in enumerate([(30, 28, 26), (26, 33, 29)]):
        cache.add(*_volume(2, 3, shape, seed=20 + i))
    kw = dict(spatial_size=(16, 16, 20), num_samples=2, batch_size=8, flip_prob=(0.5, 0.5, 0.5), rot90_prob=0.5, shift_prob=0.5,
              normalize=normalize, seed=5)
    off, old = pkg.RandCropAugment(cache, affine_prob=0.0, **kw), pkg.RandCropAugment(cache, **kw)
    on = pkg.RandCropAugment(cache, affine_prob=0.5, rotate_range=0.4, zoom_range=(0.8, 1.25), **kw)
    assert off.affine is None and old.affine is None and tuple(on.affine.shape) == (8, 16)
    outs = [_outputs(a, dev) for a in (off, old, on)]
    plain = 0
    for _ in range(3):
        for a, (x, y) in zip((off, old, on), outs):
            a(x, y)
        assert torch.equal(off.params, old.params) and torch.equal(on.params, old.params)
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        keep = on.affine[:, 0] == 0                              # an unflagged sample is what the plain gather writes, bit for bit
        assert torch.equal(outs[2][0][keep], outs[1][0][keep]) and torch.equal(outs[2][1][keep], outs[1][1][keep])
        assert bool(keep.all()) or not torch.equal(outs[2][0][~keep], outs[1][0][~keep])
        plain += int(keep.sum())
    assert 0 < plain < 24


def test_end_to_end_ct_shrunk(pkg, dev):
    cache = pkg.VolumeCache(dev)
    img, lbl = _organs(1, 1, (56, 56, 40), 14, seed=1)
    cache.add(img, lbl, scale_range=(-175, 250, 0.0, 1.0), crop_foreground=True)
    aug = pkg.RandCropAugment(cache, spatial_size=16, num_samples=4, pos=1, neg=1, flip_prob=(0.5, 0.5, 0.5), rot90_prob=0.5,
                              max_k=3, shift_prob=0.0, seed=11, affine_prob=0.7, rotate_range=(0.4, 0.4, 0.4),
                              zoom_range=(0.8, 1.25))
    x, y = _outputs(aug, dev)
    lo, hi = float(cache.image(0).min()), float(cache.image(0).max())
    images, labels = [cache.image(0)[0].cpu()], [cache.label(0)[0].cpu()]
    flagged, top = 0, 0.0
    for n in range(4):
        aug(x, y)
        on = aug.affine[:, 0] == 1
        top = max(top, float(y.max()))
        assert bool((y == y.round()).all()) and float(y.min()) >= 0 and float(y.max()) <= 13
        assert bool(torch.isfinite(x).all())
        if bool(on.any()):
            assert lo <= float(x[on].min()) and float(x[on].max()) <= hi
        xr, yr = A.apply_affine_ref(images, labels, aug.params.cpu(), aug.affine.cpu(), aug.spatial_size)
        assert torch.equal(x.cpu(), xr) and torch.equal(y.cpu(), yr)
        flagged += int(on.sum())
    assert 0 < flagged < 16 and top > 0


@pytest.mark.parametrize("normalize", NORMALIZE)
def test_affine_graph_capture_equals_eager_twin(pkg, dev, normalize):
    cache = pkg.VolumeCache(dev)
    for i, shape in enumerate([(30, 28, 26), (26, 33, 29)]):
        cache.add(*_volume(2, 3, shape, seed=20 + i))
    kw = dict(spatial_size=16, num_samples=2, batch_size=4, flip_prob=(0.5, 0.5, 0.5), rot90_prob=0.5, shift_prob=0.5,
              normalize=normalize, seed=5, affine_prob=0.6, rotate_range=(0.3, 0.0, 0.6), zoom_range=(0.75, 1.3), zoom_per_axis=True)
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
    flagged = 0
    for _ in range(3):
        graph.replay()
        twin(x2, y2)
        torch.cuda.synchronize()
        assert torch.equal(aug.params, twin.params) and torch.equal(aug.affine, twin.affine)
        assert torch.equal(x, x2) and torch.equal(y, y2)
        flagged += int(aug.affine[:, 0].sum())
    assert 0 < flagged < 12
    assert aug.state.cpu().tolist()[0] == 3


def test_affine_argument_errors(pkg, dev):
    cache = pkg.VolumeCache(dev)
    cache.add(*_volume(1, 1, (12, 12, 12), seed=1))
    mk = lambda **kw: pkg.RandCropAugment(cache, spatial_size=8, num_samples=2, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="rotate_range or zoom_range"):
        mk(affine_prob=0.5)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="affine_prob"):
            mk(affine_prob=bad, rotate_range=0.1)
    for bad in ((0.0, 1.0), (-1.0, 1.0), (1.2, 0.8)):
        with pytest.raises(ValueError, match="zoom_range"):
            mk(affine_prob=0.5, zoom_range=bad)
    with pytest.raises(ValueError, match="rotate_range"):
        mk(affine_prob=0.5, rotate_range=(0.1, 0.2))
    with pytest.raises(ValueError, match="rotate_range"):
        mk(affine_prob=0.5, rotate_range=(0.1, -0.2, 0.0))
    plain, aug = mk(), mk(affine_prob=1.0, zoom_range=(0.9, 1.1))
    assert aug.rotate_range == (0.0, 0.0, 0.0) and aug.zoom_range == (0.9, 1.1)
    x, y = _outputs(aug, dev)
    params = torch.zeros(2, 8, dtype=torch.int32)
    good = torch.tensor([A.IDENTITY_ROW, A.affine_row(zooms=(2.0, 2.0, 2.0))])
    aug.apply(params, x, y, affine=good)
    aug.apply(params, x, y)                                    # no table: no sample is flagged
    assert not bool(torch.isnan(x).any())
    with pytest.raises(ValueError, match="built with affine_prob"):
        plain.apply(params, x, y, affine=good)
    with pytest.raises(ValueError, match=r"affine \[2, 16\]"):
        aug.apply(params, x, y, affine=good[:, :12])
    for col, val, msg in ((9, float("nan"), "finite"), (4, float("inf"), "finite"), (0, 2.0, "flag"), (0, 0.5, "flag")):
        bad = good.clone()
        bad[1, col] = val
        with pytest.raises(ValueError, match=msg):
            aug.apply(params, x, y, affine=bad)
