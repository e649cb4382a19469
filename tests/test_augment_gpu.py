"""GPU checks of VolumeCache and RandCropAugment (csrc/augment.hip) against the CPU restatements of tests/augment_ref.py:
exact index lists and preprocessing, exact gathers for every flip mask x k, the sampler's params table replayed bit for bit,
its statistics, the reference CT / MR configurations end to end, graph capture and a TrainStep fed by the augment."""
import functools
import math
import struct

import pytest
import torch

import augment_ref as R

pytestmark = pytest.mark.gpu


def _volume(C, L, shape, seed, ncls=2, thr_frac=0.3):
    """image [C, *shape] float32 with exact zeros and negatives, label [L, *shape]: class ids 0..ncls-1 (L = 1) or 0/1 channels"""
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(C, *shape, generator=g)
    img[torch.rand(C, *shape, generator=g) < thr_frac] = 0.0
    if L == 1:
        lbl = torch.randint(0, ncls, (1, *shape), generator=g)
        lbl[torch.rand(1, *shape, generator=g) < 0.5] = 0
    else:
        lbl = (torch.rand(L, *shape, generator=g) < 0.2).to(torch.int64)
    return img, lbl


def _cache_volumes(cache):
    return [(tuple(s[2:]), cache.fg_indices(i).cpu().numpy(), cache.bg_indices(i).cpu().numpy()) for i, s in
            enumerate(cache.shapes)]


def _outputs(aug, dev):
    S = aug.spatial_size
    return (torch.full((aug.batch_size, aug.channels, *S), float("nan"), device=dev),
            torch.full((aug.batch_size, aug.label_channels, *S), float("nan"), device=dev))


# ---------------------------------------------------------------- VolumeCache.add
@pytest.mark.parametrize("C,L,shape,thr", [(1, 1, (7, 9, 11), 0.0), (2, 3, (17, 16, 16), 0.3), (1, 1, (16, 16, 16), 0.0),
                                           (4, 3, (33, 17, 65), -0.5), (1, 1, (1, 1, 4097), 0.0)])
def test_index_lists_exact(pkg, dev, C, L, shape, thr):
    img, lbl = _volume(C, L, shape, seed=sum(shape), ncls=5)
    cache = pkg.VolumeCache(dev, image_threshold=thr)
    i = cache.add(img, lbl)
    assert torch.equal(cache.image(i)[0].cpu(), img) and torch.equal(cache.label(i)[0].cpu(), lbl.to(torch.uint8))
    assert cache.label(i).dtype == torch.uint8 and cache.image(i).shape == (1, C, *shape)
    fg, bg = R.index_lists_ref(lbl, img, thr)
    assert torch.equal(cache.fg_indices(i).cpu().long(), fg)
    assert torch.equal(cache.bg_indices(i).cpu().long(), bg)


BIG_SCAN_SHAPE = (1, 1, 4096 * 1024 + 1)    # 1025 chunks of 4096 voxels: the smallest volume whose scan walks more than one chunk per thread


@functools.lru_cache(maxsize=None)
def _big_scan_volume():
    """image [1, *BIG_SCAN_SHAPE] with exact zeros and negatives, class ids 0..2 with about 20 % foreground; the last voxel (alone in
    the last chunk) has id 1 and an image value above every threshold used, so it ends a list whichever lists are built.  Shared by
    the tests of both list builders; nobody writes to it."""
    g = torch.Generator().manual_seed(1025)
    img = torch.randn(1, *BIG_SCAN_SHAPE, generator=g)
    img[torch.rand(1, *BIG_SCAN_SHAPE, generator=g) < 0.3] = 0.0
    r = torch.rand(1, *BIG_SCAN_SHAPE, generator=g)
    lbl = (r < 0.1).to(torch.int64) + 2 * ((r >= 0.1) & (r < 0.2)).to(torch.int64)
    lbl.view(-1)[-1] = 1
    img.view(-1)[-1] = 1.0
    return img, lbl


def test_index_lists_exact_with_more_than_1024_chunks(pkg, dev):
    """the scan's one workgroup of 1024 threads takes two chunks per thread here: threads 0..511 two each, thread 512 the last chunk
    (one voxel), the threads above it none"""
    img, lbl = _big_scan_volume()
    V = lbl.numel()
    nchunk = -(-V // 4096)
    per = -(-nchunk // 1024)
    assert nchunk == 1025 and per == 2 and -(-nchunk // per) == 513 and V - (nchunk - 1) * 4096 == 1
    cache = pkg.VolumeCache(dev, image_threshold=0.0)
    i = cache.add(img, lbl)
    fg, bg = R.index_lists_ref(lbl, img, 0.0)
    assert 0.18 * V < fg.numel() < 0.22 * V and bg.numel() > 0 and int(fg[-1]) == V - 1
    assert torch.equal(cache.fg_indices(i).cpu().long(), fg)
    assert torch.equal(cache.bg_indices(i).cpu().long(), bg)


def test_add_scale_and_crop_foreground_exact(pkg, dev):
    g = torch.Generator().manual_seed(5)
    shape = (40, 45, 37)
    img = torch.rand(1, *shape, generator=g) * 2000 - 1000
    img[:, :6] = -1000.0
    img[:, :, 40:] = -500.0
    img[:, :, :, :3] = -175.0                                  # scales to exactly 0: outside the foreground
    lbl = torch.randint(0, 14, (1, *shape), generator=g)
    cache = pkg.VolumeCache(dev)
    i = cache.add(img, lbl.float(), scale_range=(-175, 250, 0.0, 1.0), crop_foreground=True)
    s = R.scale_ref(img, -175, 250, 0.0, 1.0)
    lo, hi = R.foreground_box_ref(s)
    assert lo == [6, 0, 3] and hi == [40, 40, 37]
    sl = (slice(None),) + tuple(slice(a, b) for a, b in zip(lo, hi))
    assert torch.equal(cache.image(i)[0].cpu(), s[sl])
    assert torch.equal(cache.label(i)[0].cpu(), lbl[sl].to(torch.uint8))
    fg, bg = R.index_lists_ref(lbl[sl], s[sl])
    assert torch.equal(cache.fg_indices(i).cpu().long(), fg) and torch.equal(cache.bg_indices(i).cpu().long(), bg)
    # a_max == a_min: MONAI returns img - a_min, no clip
    j = cache.add(img, lbl, scale_range=(3.0, 3.0, 0.0, 1.0))
    assert torch.equal(cache.image(j)[0].cpu(), R.scale_ref(img, 3.0, 3.0, 0.0, 1.0))


def test_add_errors(pkg, dev):
    cache = pkg.VolumeCache(dev)
    img = torch.rand(1, 8, 8, 8) + 0.1
    with pytest.raises(ValueError, match="0..255"):
        cache.add(img, torch.full((1, 8, 8, 8), 256.0))
    with pytest.raises(ValueError, match="0..255"):
        cache.add(img, torch.full((1, 8, 8, 8), 1.5))
    with pytest.raises(ValueError, match="0..255"):
        cache.add(img, -torch.ones(1, 8, 8, 8))
    with pytest.raises(ValueError, match="foreground box is empty"):
        cache.add(-img, torch.zeros(1, 8, 8, 8), crop_foreground=True)
    with pytest.raises(ValueError, match="both empty"):
        cache.add(torch.zeros(1, 8, 8, 8), torch.zeros(1, 8, 8, 8))
    assert len(cache) == 0


def test_one_empty_list_forces_the_other(pkg, dev):
    cache = pkg.VolumeCache(dev)
    img = torch.rand(1, 12, 12, 12) + 0.1
    a = cache.add(img, torch.zeros(1, 12, 12, 12))              # no foreground: background only
    b = cache.add(img, torch.ones(1, 12, 12, 12))               # no background: foreground only
    assert cache.fg_indices(a).numel() == 0 and cache.bg_indices(a).numel() == 12 ** 3
    assert cache.bg_indices(b).numel() == 0 and cache.fg_indices(b).numel() == 12 ** 3
    aug = pkg.RandCropAugment(cache, spatial_size=4, num_samples=4, batch_size=8, pos=1, neg=1, seed=3)
    x, y = _outputs(aug, dev)
    tables = []
    for _ in range(3):
        aug(x, y)
        tables.append(aug.params.cpu().clone())
    ref = R.replay(R.aug_config(aug), _cache_volumes(cache), [0, 1], ncalls=3)
    assert all(torch.equal(t, r) for t, r in zip(tables, ref))
    assert float(y[:4].max()) == 0.0 and float(y[4:].min()) == 1.0


# ---------------------------------------------------------------- the gather with explicit tables
def _explicit_table(shapes, S, B, seed):
    g = torch.Generator().manual_seed(seed)
    rows = []
    for r in range(B):
        vol = r % len(shapes)
        dims = shapes[vol]
        corner = []
        for a in range(3):
            hi = dims[a] - S[a]
            corner.append([0, hi, int(torch.randint(0, hi + 1, (1,), generator=g))][(r + a) % 3])   # borders and inside
        flips, k = r % 8, (r // 8) % 4
        shift = r % 2
        off = float(torch.rand(1, generator=g)) * 0.2 - 0.1 if shift else 0.0
        bits = struct.unpack("<i", struct.pack("<f", off))[0]
        rows.append([vol, *corner, flips, k, shift, bits])
    return torch.tensor(rows, dtype=torch.int32)


@pytest.mark.parametrize("C,L,S,axes", [(1, 1, (12, 12, 10), (0, 1)), (4, 3, (10, 12, 12), (1, 2)), (1, 3, (9, 11, 9), (0, 2))])
def test_apply_explicit_tables(pkg, dev, C, L, S, axes):
    cache = pkg.VolumeCache(dev)
    vols = [_volume(C, L, shape, seed=i, ncls=14) for i, shape in enumerate([(37, 29, 33), (30, 41, 26), (S[0], S[1], S[2])])]
    for img, lbl in vols:
        cache.add(img, lbl)
    images = [cache.image(i)[0].cpu() for i in range(3)]
    labels = [cache.label(i)[0].cpu() for i in range(3)]
    B = 32                                                     # every flip mask x k, shift on and off
    table = _explicit_table([s[2:] for s in cache.shapes], S, B, seed=C + L)
    for normalize in (None, "nonzero_channel_wise"):
        aug = pkg.RandCropAugment(cache, spatial_size=S, num_samples=4, batch_size=B, spatial_axes=axes, normalize=normalize)
        x, y = _outputs(aug, dev)
        aug.apply(table, x, y)
        xr, yr = R.apply_ref(images, labels, table, S, axes, normalize=normalize is not None)
        assert torch.equal(y.cpu(), yr)
        if normalize is None:
            assert torch.equal(x.cpu(), xr)
        else:
            err = float((x.cpu() - xr).abs().max())
            assert err <= 1e-6 * float(xr.abs().max()), err
        x2, y2 = _outputs(aug, dev)
        aug.apply(table.to(dev), x2, y2)
        assert torch.equal(x, x2) and torch.equal(y, y2)       # run to run bit-identical
    with pytest.raises(ValueError, match="leaves the volume"):
        bad = table.clone()
        bad[0, 1] = cache.shapes[int(bad[0, 0])][2] - S[0] + 1
        aug.apply(bad, x, y)


# ---------------------------------------------------------------- the sampler
@pytest.mark.parametrize("sampling", ["pos_neg", "uniform"])
def test_sampler_replays_bit_for_bit(pkg, dev, sampling):
    cache = pkg.VolumeCache(dev)
    for i, shape in enumerate([(20, 18, 25), (16, 30, 16), (40, 17, 19)]):
        cache.add(*_volume(1, 1, shape, seed=10 + i, ncls=3))
    aug = pkg.RandCropAugment(cache, spatial_size=(8, 8, 6), num_samples=4, batch_size=8, pos=3, neg=1, sampling=sampling,
                              flip_prob=(0.3, 0.5, 0.7), rot90_prob=0.5, max_k=3, shift_offsets=0.1, shift_prob=0.5, seed=1234)
    x, y = _outputs(aug, dev)
    vols = _cache_volumes(cache)
    cfg = R.aug_config(aug)
    order = [2, 0, 1, 2, 1]
    aug.set_order(order)
    got = []
    for _ in range(6):
        aug(x, y)
        got.append(aug.params.cpu().clone())
    ref = R.replay(cfg, vols, order, ncalls=6)
    for n, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(a, b), (n, a, b)
    assert aug.state.cpu().tolist() == [6, (6 * 2) % 5, 5, 0]
    aug.reset(call=1000)
    aug(x, y)
    assert torch.equal(aug.params.cpu(), R.replay(cfg, vols, order, ncalls=1, call=1000)[0])
    xr, yr = R.apply_ref([cache.image(i)[0].cpu() for i in range(3)], [cache.label(i)[0].cpu() for i in range(3)],
                         aug.params.cpu(), aug.spatial_size)
    assert torch.equal(x.cpu(), xr) and torch.equal(y.cpu(), yr)


def test_sampler_statistics(pkg, dev):
    """20k samples per configuration at a fixed seed: each drawn share within 5 sigma of its probability"""
    shape, S = (24, 24, 24), 8
    g = torch.Generator().manual_seed(0)
    img = torch.zeros(1, *shape)
    img[:, 4:21, 4:21, 4:21] = torch.rand(1, 17, 17, 17, generator=g) + 0.5     # every candidate centre needs no correction
    lbl = torch.zeros(1, *shape)
    lbl[:, 4:21, 4:21, 4:21] = (torch.rand(1, 17, 17, 17, generator=g) < 0.3).float()
    cache = pkg.VolumeCache(dev)
    cache.add(img, lbl)
    lab = lbl[0].bool()

    def within(count, n, p):
        return abs(count / n - p) <= 5 * math.sqrt(p * (1 - p) / n) + 1e-12

    for pos, neg in ((1, 1), (3, 1)):
        aug = pkg.RandCropAugment(cache, spatial_size=S, num_samples=4, batch_size=4000, pos=pos, neg=neg,
                                  flip_prob=(0.1, 0.3, 0.5), rot90_prob=0.4, max_k=3, shift_offsets=0.1, shift_prob=0.5, seed=99)
        x, y = _outputs(aug, dev)
        rows = []
        for _ in range(5):
            aug(x, y)
            rows.append(aug.params.cpu().clone())
        t = torch.cat(rows).long()
        n = t.shape[0]
        c = t[:, 1:4] + S // 2
        is_pos = lab[c[:, 0], c[:, 1], c[:, 2]]
        assert within(int(is_pos.sum()), n, pos / (pos + neg))
        for a, p in enumerate((0.1, 0.3, 0.5)):
            assert within(int((t[:, 4] >> a & 1).sum()), n, p)
        rot = t[:, 5] > 0
        assert within(int(rot.sum()), n, 0.4)
        for k in (1, 2, 3):
            assert within(int((t[rot, 5] == k).sum()), int(rot.sum()), 1 / 3)
        sh = t[:, 6] == 1
        assert within(int(sh.sum()), n, 0.5)
        off = torch.tensor([struct.unpack("<f", struct.pack("<i", int(b)))[0] for b in t[:, 7].tolist()], dtype=torch.float64)
        assert bool((off[~sh] == 0).all()) and float(off[sh].min()) >= -0.1 and float(off[sh].max()) < 0.1
        assert abs(float(off[sh].mean())) <= 5 * 0.2 / math.sqrt(12 * int(sh.sum()))
        assert float(off[sh].min()) < -0.09 and float(off[sh].max()) > 0.09


# ---------------------------------------------------------------- the reference configurations
def _organs(C, L, shape, ncls, seed):
    """a body-like synthetic volume: intensity blobs on a background, labels as nested spheres"""
    g = torch.Generator().manual_seed(seed)
    zz, yy, xx = torch.meshgrid(*[torch.linspace(-1, 1, s) for s in shape], indexing="ij")
    r = (zz ** 2 + yy ** 2 + xx ** 2).sqrt()
    img = (torch.randn(C, *shape, generator=g) * 50 + 300 * (r < 0.9).float() - 200).float()
    if L == 1:
        lbl = torch.zeros(1, *shape)
        for c in range(1, ncls):
            cz, cy, cx = (torch.rand(3, generator=g) * 1.2 - 0.6).tolist()
            lbl[0][((zz - cz) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2).sqrt() < 0.08 + 0.02 * (c % 4)] = c
    else:
        lbl = torch.stack([(r < 0.2 + 0.1 * c).float() for c in range(L)])
    return img, lbl


@pytest.mark.parametrize("case", ["ct", "mr"])
def test_end_to_end_reference_configs(pkg, dev, case):
    cache = pkg.VolumeCache(dev)
    if case == "ct":
        img, lbl = _organs(1, 1, (320, 320, 200), 14, seed=1)
        cache.add(img, lbl, scale_range=(-175, 250, 0.0, 1.0), crop_foreground=True)
        aug = pkg.RandCropAugment(cache, spatial_size=96, num_samples=4, pos=1, neg=1, flip_prob=(0.5, 0.5, 0.5),
                                  rot90_prob=0.5, max_k=3, shift_offsets=0.1, shift_prob=0.5, seed=11)
    else:
        img, lbl = _organs(4, 3, (240, 240, 155), 0, seed=2)
        cache.add(img, lbl)
        aug = pkg.RandCropAugment(cache, spatial_size=128, num_samples=4, pos=1, neg=1, flip_prob=(0.5, 0.5, 0.5),
                                  rot90_prob=0.5, shift_offsets=0.1, shift_prob=1.0, normalize="nonzero_channel_wise", seed=12)
    x, y = _outputs(aug, dev)
    images, labels = [cache.image(0)[0].cpu()], [cache.label(0)[0].cpu()]
    for n in range(2):
        aug(x, y)
        p = aug.params.cpu()
        assert torch.equal(p, R.replay(R.aug_config(aug), _cache_volumes(cache), [0], ncalls=1, call=n)[0])
        xr, yr = R.apply_ref(images, labels, p, aug.spatial_size, normalize=aug.normalize is not None)
        assert torch.equal(y.cpu(), yr)
        if aug.normalize is None:
            assert torch.equal(x.cpu(), xr)
        else:
            assert float((x.cpu() - xr).abs().max()) <= 1e-6 * float(xr.abs().max())


# ---------------------------------------------------------------- capture and the training step
@pytest.mark.parametrize("normalize", [None, "nonzero_channel_wise"])
def test_graph_capture_equals_eager_twin(pkg, dev, normalize):
    cache = pkg.VolumeCache(dev)
    for i, shape in enumerate([(30, 28, 26), (26, 33, 29)]):
        cache.add(*_volume(2, 3, shape, seed=20 + i))
    kw = dict(spatial_size=16, num_samples=2, batch_size=4, flip_prob=(0.5, 0.5, 0.5), rot90_prob=0.5, shift_prob=0.5,
              normalize=normalize, seed=5)
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
    for _ in range(4):
        graph.replay()
        twin(x2, y2)
        torch.cuda.synchronize()
        assert torch.equal(aug.params, twin.params)
        assert torch.equal(x, x2) and torch.equal(y, y2)
    assert aug.state.cpu().tolist()[0] == 4


def test_feeds_train_step(pkg, dev):
    C1 = dict(in_channels=1, out_channels=2, img_size=(32, 32, 32), feature_size=16, hidden_size=128, mlp_dim=512,
              num_heads=4, pos_embed="perceptron", norm_name="instance", res_block=True)
    cache = pkg.VolumeCache(dev)
    img, lbl = _organs(1, 1, (64, 60, 48), 2, seed=3)
    cache.add(img, lbl, scale_range=(-175, 250, 0.0, 1.0), crop_foreground=True)
    aug = pkg.RandCropAugment(cache, spatial_size=32, num_samples=2, pos=1, neg=1, seed=0)
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
        aug(x, y)
        step.run()
        torch.cuda.synchronize()
        assert not torch.equal(x, prev)
        prev = x.clone()
        assert math.isfinite(float(step.loss.detach()))
