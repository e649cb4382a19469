"""GPU checks of class-balanced crop sampling (csrc/augment.hip: the class count / scan / scatter trio and the sampler's class
branch) against tests/augment_classes_ref.py: the per-class voxel lists exact with their order, the sampler's params table and
class record replayed bit for bit, the other Philox blocks untouched, the crops end to end, device ratios steering a captured
graph, and what the public surface refuses."""
import numpy as np
import pytest
import torch

import augment_classes_ref as K
import augment_ref as R
from test_augment_classes_cpu import FREQ_RATIOS, FREQ_SEED
from test_augment_gpu import _big_scan_volume, _outputs

pytestmark = pytest.mark.gpu
THR = 0.25
CHUNK = 4096


def _image(C, shape, seed):
    """float32 with exact zeros, values either side of THR and negatives"""
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(C, *shape, generator=g)
    img[torch.rand(C, *shape, generator=g) < 0.4] = 0.0
    return img


def _ids(shape, hi, seed, absent=()):
    g = torch.Generator().manual_seed(seed)
    lbl = torch.randint(0, hi, (1, *shape), generator=g)
    for c in absent:
        lbl[lbl == c] = 0
    return lbl


def _btcv_like():
    """(33, 17, 65), K = 14: ids up to 16 (14..16 are in no list), classes 3 and 7 absent, class 11 only in the last chunk"""
    shape = (33, 17, 65)
    lbl = _ids(shape, 17, seed=4, absent=(3, 7, 11))
    flat = lbl.view(-1)
    V = flat.numel()
    last = (V - 1) // CHUNK * CHUNK
    assert V - last < CHUNK and last > 0
    flat[torch.tensor([last, last + 1, last + 300, V - 1])] = 11
    return shape, lbl, 14


def _list_cases():
    one = torch.full((1, 9, 9, 9), 2)
    multi = (torch.rand(3, 17, 16, 16, generator=torch.Generator().manual_seed(3)) < 0.4).to(torch.int64)
    return {
        "partial-chunk": ((7, 9, 11), _ids((7, 9, 11), 5, seed=1), 5, 1),
        "past-chunk-edge": ((1, 1, 4097), _ids((1, 1, 4097), 3, seed=2), 3, 1),
        "multi-label": ((17, 16, 16), multi * 3, None, 2),
        "btcv-like": (*_btcv_like(), 2),
        "k32": ((16, 16, 16), _ids((16, 16, 16), 32, seed=5), 32, 1),
        "one-class": ((9, 9, 9), one, 4, 1),
    }


LIST_CASES = _list_cases()


@pytest.mark.parametrize("image_mask", [False, True])
@pytest.mark.parametrize("name", list(LIST_CASES))
def test_class_lists_exact(pkg, dev, name, image_mask):
    shape, lbl, num_classes, C = LIST_CASES[name]
    img = _image(C, shape, seed=len(name))
    cache = pkg.VolumeCache(dev, image_threshold=THR)
    i = cache.add(img, lbl)
    cache.build_class_indices(num_classes, image_mask=image_mask)
    ref = K.class_index_lists_ref(lbl.numpy(), img.numpy(), num_classes, image_mask, THR)
    counts = cache.class_counts(i)
    assert counts == [len(a) for a in ref]
    if name == "btcv-like":
        assert counts[3] == 0 and counts[7] == 0 and (image_mask or counts[11] == 4)
    if name == "one-class" and not image_mask:
        assert counts == [0, 0, 9 ** 3, 0]
    for c, a in enumerate(ref):
        got = cache.class_indices(i, c)
        assert got.dtype == torch.int32 and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), a), (name, c)
    off = cache.class_offsets(i)
    assert off.dtype == torch.int64 and off.cpu().tolist() == [0, *np.cumsum(counts).tolist()]
    table = cache.class_table()
    assert table.dtype == torch.int64 and tuple(table.shape) == (1, 2)
    assert table.cpu().tolist()[0][1] == off.data_ptr()
    assert tuple(cache.table().shape) == (1, 12)                 # the volume table does not move


def test_class_lists_exact_with_more_than_1024_chunks(pkg, dev):
    """test_augment_gpu's volume of 1025 chunks: every class's scan walks two chunks per thread, the last chunk holds one voxel"""
    img, lbl = _big_scan_volume()
    V = lbl.numel()
    assert -(-V // CHUNK) == 1025 and int(lbl.view(-1)[-1]) == 1 and float(img.view(-1)[-1]) > THR
    cache = pkg.VolumeCache(dev, image_threshold=THR)
    i = cache.add(img, lbl)
    for image_mask in (False, True):
        cache.build_class_indices(3, image_mask=image_mask)
        ref = K.class_index_lists_ref(lbl.numpy(), img.numpy(), 3, image_mask, THR)
        counts = cache.class_counts(i)
        assert counts == [len(a) for a in ref] and all(counts) and int(ref[1][-1]) == V - 1
        for c, a in enumerate(ref):
            assert np.array_equal(cache.class_indices(i, c).cpu().numpy(), a), (image_mask, c)
        assert cache.class_offsets(i).cpu().tolist() == [0, *np.cumsum(counts).tolist()]


def test_lists_of_volumes_added_later(pkg, dev):
    cache = pkg.VolumeCache(dev)
    a = cache.add(_image(1, (7, 9, 11), 0), _ids((7, 9, 11), 5, seed=1))
    cache.build_class_indices(5)
    lbl = _ids((9, 8, 7), 5, seed=2, absent=(3,))
    b = cache.add(_image(1, (9, 8, 7), 1), lbl)
    ref = K.class_index_lists_ref(lbl.numpy(), np.zeros((1, 9, 8, 7)), 5)
    assert cache.class_counts(b) == [len(r) for r in ref] and cache.class_counts(b)[3] == 0
    assert all(np.array_equal(cache.class_indices(b, c).cpu().numpy(), ref[c]) for c in range(5))
    assert tuple(cache.class_table().shape) == (2, 2) and sum(cache.class_counts(a)) == 7 * 9 * 11


# ---------------------------------------------------------------- the sampler
def _two_volumes(pkg, dev):
    """volumes (12, 10, 9) and (9, 12, 11), five classes; the second lacks classes 2 and 4"""
    cache = pkg.VolumeCache(dev)
    labels = [_ids((12, 10, 9), 5, seed=1), _ids((9, 12, 11), 5, seed=2, absent=(2, 4))]
    for j, lbl in enumerate(labels):
        cache.add(_image(1, tuple(lbl.shape[1:]), 30 + j), lbl)
    return cache, labels


def _class_volumes(cache, k):
    return [(tuple(s[2:]), [cache.class_indices(i, c).cpu().numpy() for c in range(k)]) for i, s in enumerate(cache.shapes)]


SAMPLER_KW = dict(spatial_size=(8, 8, 6), num_samples=4, batch_size=8, sampling="label_classes", num_classes=5,
                  flip_prob=(0.3, 0.5, 0.7), rot90_prob=0.5, max_k=3, shift_offsets=0.1, shift_prob=0.5, seed=FREQ_SEED)


def test_sampler_replays_bit_for_bit(pkg, dev):
    cache, labels = _two_volumes(pkg, dev)
    aug = pkg.RandCropAugment(cache, class_ratios=FREQ_RATIOS, **SAMPLER_KW)
    assert cache.class_counts(1)[2] == 0 and cache.class_counts(1)[4] == 0 and min(cache.class_counts(0)) > 0
    assert aug.class_ratios.cpu().tolist() == [0.0, 1.0, 2.0, 1.0, 3.0] and tuple(aug.classes.shape) == (8,)
    x, y = _outputs(aug, dev)
    order = [1, 0, 1, 0, 0]
    aug.set_order(order)
    got = []
    for _ in range(3):
        aug(x, y)
        got.append((aug.params.cpu().clone(), aug.classes.cpu().clone()))
    tables, classes = K.replay_classes(R.aug_config(aug), _class_volumes(cache, 5), FREQ_RATIOS, order, ncalls=3)
    for n, ((p, c), pr, cr) in enumerate(zip(got, tables, classes)):
        assert torch.equal(p, pr), (n, p, pr)
        assert torch.equal(c, cr), (n, c, cr)
    drawn = torch.cat([c for _, c in got])
    vols = torch.cat([p[:, 0] for p, _ in got])
    assert int((drawn == 0).sum()) == 0 and not bool(((vols == 1) & ((drawn == 2) | (drawn == 4))).any())
    assert aug.state.cpu().tolist() == [3, (3 * 2) % 5, 5, 0]    # counter and cursor advance as in the other modes


def test_other_blocks_untouched(pkg, dev):
    cache, _ = _two_volumes(pkg, dev)
    kw = {k: v for k, v in SAMPLER_KW.items() if k not in ("sampling", "num_classes")}
    extra = dict(affine_prob=0.5, rotate_range=0.4, zoom_range=(0.8, 1.2), intensity=pkg.IntensityAugment.nnunet())
    a = pkg.RandCropAugment(cache, sampling="label_classes", num_classes=5, class_ratios=FREQ_RATIOS, **kw, **extra)
    b = pkg.RandCropAugment(cache, sampling="pos_neg", **kw, **extra)
    xa, ya = _outputs(a, dev)
    xb, yb = _outputs(b, dev)
    corners_differ = flagged = False
    for _ in range(3):
        a(xa, ya)
        b(xb, yb)
        assert torch.equal(a.affine, b.affine) and torch.equal(a.intensity, b.intensity)
        assert torch.equal(a.params[:, 0], b.params[:, 0]) and torch.equal(a.params[:, 4:], b.params[:, 4:])
        corners_differ |= not torch.equal(a.params[:, 1:4], b.params[:, 1:4])
        flagged |= bool(a.affine[:, 0].any()) and bool(a.intensity[:, 0].any())
    assert corners_differ and flagged
    assert a.state.cpu().tolist() == b.state.cpu().tolist()


def test_end_to_end_crops_hold_their_class(pkg, dev):
    cache, _ = _two_volumes(pkg, dev)
    aug = pkg.RandCropAugment(cache, class_ratios=FREQ_RATIOS, **SAMPLER_KW)
    x, y = _outputs(aug, dev)
    x2, y2 = _outputs(aug, dev)
    for _ in range(2):
        aug(x, y)
        cls = aug.classes.cpu().tolist()
        assert all(c in (1, 2, 3, 4) for c in cls)
        for s, c in enumerate(cls):
            assert bool((y[s] == c).any()), (s, c)
        aug.apply(aug.params, x2, y2)
        assert torch.equal(x, x2) and torch.equal(y, y2)
    xr, yr = R.apply_ref([cache.image(i)[0].cpu() for i in range(2)], [cache.label(i)[0].cpu() for i in range(2)],
                         aug.params.cpu(), aug.spatial_size)
    assert torch.equal(x.cpu(), xr) and torch.equal(y.cpu(), yr)


def test_device_ratios_steer_a_captured_graph(pkg, dev):
    cache, _ = _two_volumes(pkg, dev)
    aug = pkg.RandCropAugment(cache, class_ratios=FREQ_RATIOS, **SAMPLER_KW)
    x, y = _outputs(aug, dev)
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
    cfg, vols = R.aug_config(aug), _class_volumes(cache, 5)

    def replays(ratios, n, call):
        out = []
        for _ in range(n):
            graph.replay()
            torch.cuda.synchronize()
            out.append((aug.params.cpu().clone(), aug.classes.cpu().clone()))
        tables, classes = K.replay_classes(cfg, vols, ratios, [0, 1], ncalls=n, call=call)
        for (p, c), pr, cr in zip(out, tables, classes):
            assert torch.equal(p, pr) and torch.equal(c, cr), (call, c, cr)
        return out

    replays(FREQ_RATIOS, 3, call=0)
    new = [5.0, 0.0, 0.0, 0.25, 0.0]
    aug.class_ratios.copy_(torch.tensor(new, device=dev))        # on the device, no rebuild, no recapture
    out = replays(new, 2, call=3)
    assert all(set(c.tolist()) <= {0, 3} for _, c in out)
    aug.set_class_ratios(torch.tensor([0.0, float("nan"), -1.0, 0.0, float("inf")], device=dev))    # unchecked: all count as 0
    for p, c in replays([0.0] * 5, 2, call=5):
        assert c.tolist() == [-1] * 8
        for row in p.tolist():
            dims = cache.shapes[row[0]][2:]
            assert all(0 <= z and z + s <= d for z, s, d in zip(row[1:4], aug.spatial_size, dims))
    assert aug.state.cpu().tolist()[0] == 7


# ---------------------------------------------------------------- what the surface refuses
def test_errors(pkg, dev):
    cache, _ = _two_volumes(pkg, dev)
    kw = {k: v for k, v in SAMPLER_KW.items() if k != "num_classes"}
    with pytest.raises(ValueError, match="num_classes is required"):
        pkg.RandCropAugment(cache, **kw)
    with pytest.raises(ValueError, match="num_classes is required"):
        cache.build_class_indices()
    with pytest.raises(ValueError, match="1..32"):
        pkg.RandCropAugment(cache, num_classes=33, **kw)
    with pytest.raises(ValueError, match="1..32"):
        cache.build_class_indices(33)
    with pytest.raises(ValueError, match="5 values"):
        pkg.RandCropAugment(cache, num_classes=5, class_ratios=[1, 1, 1], **kw)
    with pytest.raises(ValueError, match="finite and nonnegative"):
        pkg.RandCropAugment(cache, num_classes=5, class_ratios=[1, 1, -1, 1, 1], **kw)
    with pytest.raises(ValueError, match="volume 1 holds no voxel"):
        pkg.RandCropAugment(cache, num_classes=5, class_ratios=[0, 0, 1, 0, 1], **kw)
    aug = pkg.RandCropAugment(cache, num_classes=5, **kw)
    assert aug.class_ratios.cpu().tolist() == [1.0] * 5          # the default
    with pytest.raises(ValueError, match="volume 1 holds no voxel"):
        aug.set_class_ratios([0, 0, 1, 0, 1])
    with pytest.raises(ValueError, match="finite and nonnegative"):
        aug.set_class_ratios(torch.tensor([1.0, float("inf"), 1.0, 1.0, 1.0]))
    with pytest.raises(ValueError, match="5 values"):
        aug.set_class_ratios(torch.ones(4, device=dev))
    assert aug.class_ratios.cpu().tolist() == [1.0] * 5          # a refused update changes nothing
    with pytest.raises(ValueError, match='sampling="label_classes"'):
        pkg.RandCropAugment(cache, spatial_size=(8, 8, 6), num_samples=4).set_class_ratios([1] * 5)
    multi = pkg.VolumeCache(dev)
    multi.add(_image(2, (9, 9, 9), 0), (torch.rand(3, 9, 9, 9) < 0.5).to(torch.int64))
    with pytest.raises(ValueError, match="None or 3"):
        pkg.RandCropAugment(multi, spatial_size=4, num_samples=2, sampling="label_classes", num_classes=4)
    with pytest.raises(ValueError, match="None or 3"):
        multi.build_class_indices(4)
    assert pkg.RandCropAugment(multi, spatial_size=4, num_samples=2, sampling="label_classes").num_classes == 3
