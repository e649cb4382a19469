"""The morphology module on the GPU against scipy (tests/morphology_ref.py), bit for bit; inputs, outputs and the packed
workspace live inside red zones (tests/guard.py), so a store outside a buffer, an output voxel that unpack did not write and
a padding bit of a row's last word that was trusted all show."""
import functools

import numpy as np
import pytest
import torch

import morphology_ref as ref
from guard import Guard

pytestmark = pytest.mark.gpu

K, T = 4, 8                                                      # = morphology.MORPH_FUSED, MORPH_TILE (asserted below)
SHAPES = [(1, 1, 5, 7, 67), (2, 3, 17, 9, 130), (1, 1, 3, 3, 64), (1, 2, 4, 5, 1),
          (1, 1, T + 1, 2 * T + 1, 70)]                          # the last one crosses the tile in z and in y
ITERATIONS = [1, 2, K, K + 1, 2 * K + 1]                         # the last three cross the launch batching
DTYPES = [torch.float32, torch.uint8, torch.bool]
REF = {"dilation": ref.dilation, "erosion": ref.erosion, "opening": ref.opening, "closing": ref.closing}


def rand_mask(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def on_device(pkg, dev, name, m, dtype=torch.float32, **kw):
    out = getattr(pkg, name)(torch.from_numpy(m).to(dtype).to(dev), **kw)
    assert out.dtype == dtype and out.shape == m.shape
    return out.cpu().to(torch.uint8).numpy()


@functools.lru_cache(maxsize=None)
def picked(shape, op, connectivity, border, iterations):
    """(mask, reference, whether the reference is neither empty nor full).  Masks are tried from dense to a single voxel
    (dilation) or from nearly full to a single missing voxel (erosion), that voxel at a corner, until the reference is neither
    empty nor full; when not even the last one is, it is used as it is.  Dilation and erosion are monotone, so when the
    dilation of the empty mask is already full (border 1 reaches every voxel), or the erosion of the full mask already empty
    (border 0 does), no mask has a reference in between: such a case still runs, on a random mask."""
    fn = REF[op]
    grow = op == "dilation"
    extreme = fn(np.full(shape, 0 if grow else 1, np.uint8), iterations, connectivity, border)
    if extreme.all() if grow else not extreme.any():
        m = rand_mask(shape, 0.3 if grow else 0.9, 1)
        return m, fn(m, iterations, connectivity, border), False
    single = np.full(shape, 0 if grow else 1, np.uint8)
    single[..., 0, 0, 0] = 1 - single[..., 0, 0, 0]
    for m in [rand_mask(shape, d if grow else 1 - d, 2) for d in (0.3, 0.03, 0.003)] + [single]:
        want = fn(m, iterations, connectivity, border)
        if 0 < want.sum() < want.size:
            return m, want, True
    return m, want, False                                        # not even one voxel at a corner lands in between


@pytest.mark.parametrize("connectivity", [1, 2, 3])
@pytest.mark.parametrize("op", ["dilation", "erosion"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_masks_against_scipy(pkg, dev, shape, op, connectivity):
    assert (pkg.morphology.MORPH_FUSED, pkg.morphology.MORPH_TILE) == (K, T)
    informative = 0
    with Guard(dev) as gd:
        for border in (0, 1):
            for n in ITERATIONS:
                m, want, between = picked(shape, op, connectivity, border, n)
                print(f"{op} {shape} c{connectivity} b{border} n{n}: mask {int(m.sum())}, reference {int(want.sum())} of {want.size}")
                if between:
                    assert 0 < want.sum() < want.size
                    informative += 1
                for dtype in DTYPES:
                    got = on_device(pkg, dev, "binary_" + op, m, dtype, iterations=n, connectivity=connectivity, border_value=border)
                    assert np.array_equal(got, want), (border, n, dtype)
    assert gd.check() > 0
    assert informative >= 2                                      # every shape has cases in between under at least one border


@pytest.mark.parametrize("W", [65, 128])
def test_placed_voxels(pkg, dev, W):
    D, H = 5, 6
    spots = [(z, y, x) for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)] + [(2, 3, 63), (2, 3, 64), (1, 2, W - 1)]
    m = np.zeros((1, len(spots), D, H, W), np.uint8)
    for c, (z, y, x) in enumerate(spots):
        m[0, c, z, y, x] = 1
    with Guard(dev) as gd:
        for connectivity in (1, 2, 3):
            for n in (1, 2):
                want = ref.dilation(m, n, connectivity)
                assert 0 < want.sum() < want.size
                assert np.array_equal(on_device(pkg, dev, "binary_dilation", m, iterations=n, connectivity=connectivity), want)
                assert np.array_equal(on_device(pkg, dev, "binary_erosion", 1 - m, torch.uint8, iterations=n, connectivity=connectivity,
                                                border_value=1), 1 - want)
    assert gd.check() > 0


@pytest.mark.parametrize("W", [64, 70])
def test_full_volume_and_full_last_word(pkg, dev, W):
    full = np.ones((1, 2, 6, 9, W), np.uint8)
    last = np.zeros((1, 1, 3, 4, 70), np.uint8)
    last[..., 64:] = 1                                           # the last word's six voxels, all set: padding bits must not leak
    with Guard(dev) as gd:
        for connectivity in (1, 2, 3):
            for n in (1, 2):
                assert on_device(pkg, dev, "binary_erosion", full, iterations=n, connectivity=connectivity, border_value=1).all()
                got = on_device(pkg, dev, "binary_erosion", full, iterations=n, connectivity=connectivity, border_value=0)
                want = ref.erosion(full, n, connectivity, 0)
                assert np.array_equal(got, want) and want.sum() == 2 * (6 - 2 * n) * (9 - 2 * n) * (W - 2 * n)
                for border in (0, 1):
                    for op in ("dilation", "erosion"):
                        got = on_device(pkg, dev, "binary_" + op, last, torch.uint8, iterations=n, connectivity=connectivity, border_value=border)
                        assert np.array_equal(got, REF[op](last, n, connectivity, border)), (op, n, border)
    assert gd.check() > 0


def test_class_id_inside_the_pack(pkg, dev):
    """the mask of one class of a class-id map, taken inside the pack pass"""
    ids = np.random.default_rng(4).integers(0, 4, (2, 1, 6, 7, 67)).astype(np.float32)
    mm = pkg.morphology
    for dtype in (torch.float32, torch.uint8):
        got = mm._morph(torch.from_numpy(ids).to(dtype).to(dev), mm._DILATE, 1, 2, 0, "test", class_id=2)
        assert np.array_equal(got.cpu().numpy().astype(np.uint8), ref.dilation(ids == 2, 1, 2))


@pytest.mark.parametrize("op", ["opening", "closing"])
@pytest.mark.parametrize("shape", SHAPES[:2] + SHAPES[4:], ids=lambda s: "x".join(map(str, s)))
def test_opening_and_closing(pkg, dev, shape, op):
    m = rand_mask(shape, 0.97 if op == "opening" else 0.05, 7)
    with Guard(dev) as gd:
        for connectivity in (1, 2, 3):
            for n in (1, 3):
                want = REF[op](m, n, connectivity)
                for dtype in DTYPES:
                    assert np.array_equal(on_device(pkg, dev, "binary_" + op, m, dtype, iterations=n, connectivity=connectivity), want)
        want = REF[op](m, 1, 1)
        assert 0 < want.sum() < want.size and not np.array_equal(want, m)
    assert gd.check() > 0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_contour(pkg, dev, shape):
    m = rand_mask(shape, 0.9, 8)
    with Guard(dev) as gd:
        for connectivity in (1, 2, 3):
            want = m & (1 - ref.erosion(m, 1, connectivity, 0))
            assert np.array_equal(want, ref.contour(m, connectivity)) and want.any()
            for dtype in DTYPES:
                assert np.array_equal(on_device(pkg, dev, "binary_contour", m, dtype, connectivity=connectivity), want)
    assert gd.check() > 0


def test_decollated_and_untouched_input(pkg, dev):
    m = rand_mask((2, 5, 6, 70), 0.4, 9)
    x = torch.from_numpy(m).float().to(dev)
    keep = x.clone()
    out = pkg.binary_dilation(x, iterations=2, connectivity=2)
    assert out.shape == x.shape and torch.equal(x, keep)
    assert np.array_equal(out.cpu().numpy(), ref.dilation(m[None], 2, 2)[0])
    strided = torch.from_numpy(rand_mask((1, 1, 6, 70, 5), 0.4, 10)).to(dev).permute(0, 1, 4, 2, 3)      # not contiguous
    assert np.array_equal(pkg.binary_fill_holes(strided).cpu().numpy(), ref.fill_holes(strided.cpu().numpy()))


# --------------------------------------------------------------------------------------------------------- hole filling
def hollow_box():
    m = np.zeros((1, 1, 9, 9, 70), np.uint8)
    m[0, 0, 2:7, 2:7, 2:68] = 1
    m[0, 0, 3:6, 3:6, 3:67] = 0
    return m


def test_fill_holes_boxes(pkg, dev):
    box = hollow_box()
    tunnel = box.copy()
    tunnel[0, 0, 2, 4, 10] = 0                       # through the middle of a wall: open under every connectivity
    diagonal = box.copy()
    diagonal[0, 0, 2, 2, 10] = 0                     # an edge voxel of the shell: touches the cavity's (3, 3, 10) only diagonally
    with Guard(dev) as gd:
        for connectivity in (1, 2, 3):
            for m, filled in ((box, 576), (tunnel, 0), (diagonal, 576 if connectivity == 1 else 0)):
                want = ref.fill_holes(m, connectivity)
                assert want.sum() - m.sum() == filled
                for dtype in DTYPES:
                    assert np.array_equal(on_device(pkg, dev, "binary_fill_holes", m, dtype, connectivity=connectivity), want)
    assert gd.check() > 0


def test_fill_holes_random_and_batched(pkg, dev):
    m = rand_mask((2, 3, 17, 9, 67), 0.6, 11)
    two = np.concatenate([hollow_box(), hollow_box()])
    two[1, 0, 3:6, 3:6, 30] = 1                      # the second item's cavity is split in two, and one half is open
    two[1, 0, 2, 4, 50] = 0
    with Guard(dev) as gd:
        for connectivity in (1, 2, 3):
            want = ref.fill_holes(m, connectivity)
            assert want.sum() > m.sum() or connectivity > 1      # at density 0.6 the complement is one component under 18 / 26
            assert np.array_equal(on_device(pkg, dev, "binary_fill_holes", m, connectivity=connectivity), want)
            want = ref.fill_holes(two, connectivity)
            assert want[0].sum() - two[0].sum() == 576 and want[1].sum() - two[1].sum() == 3 * 3 * 27
            assert np.array_equal(on_device(pkg, dev, "binary_fill_holes", two, torch.bool, connectivity=connectivity), want)
    assert gd.check() > 0


def class_map_cases():
    ids = np.zeros((4, 1, 13, 13, 70), np.float32)
    ids[:, 0, 1:12, 1:12, 1:69] = 2
    ids[:, 0, 3:10, 3:10, 3:67] = 1
    ids[0, 0, 6, 6, 6] = 0                           # the nest: a hole inside label 1, label 1 inside label 2
    ids[0, 0, 5:8, 5:8, 62:66] = 0
    ids[1, 0, 2, 5, 5] = 0                           # bordered by labels 1 and 2
    ids[2, 0, 6, 6, 1:40] = 0                        # a tunnel through both labels to the background at the face x = 0
    ids[3, 0, 1, 6, 6] = 0                           # (0, 6, 6) is background: joins the outside, which touches the faces
    ids[3, 0, 10, 10, 60] = 0                        # wholly inside label 2 under connectivity 1; label 1 is a diagonal neighbour
    return ids


def test_fill_holes_transform(pkg, dev):
    ids = class_map_cases()
    x = torch.from_numpy(ids).to(dev)
    with Guard(dev) as gd:
        for connectivity in (None, 1, 2, 3):
            for applied in (None, [1], [2], [1, 2, 5]):
                want = ref.fill_holes_rule(ids, applied, connectivity)
                got = pkg.FillHoles(applied, connectivity)(x)
                assert got.dtype == x.dtype and np.array_equal(got.cpu().numpy(), want), (connectivity, applied)
                got8 = pkg.FillHoles(applied, connectivity)(x.to(torch.uint8))
                assert got8.dtype == torch.uint8 and np.array_equal(got8.cpu().numpy(), want.astype(np.uint8))
        want = ref.fill_holes_rule(ids, None, None)
        assert want[0, 0, 6, 6, 6] == 1 and (want[0, 0, 5:8, 5:8, 62:66] == 1).all()      # the nest fills with the inner label
        assert want[1, 0, 2, 5, 5] == 0                                                    # two labels around it
        assert (want[2, 0, 6, 6, :40] == 0).all()                                          # reaches a face
        assert ref.fill_holes_rule(ids, [2], None)[0, 0, 6, 6, 6] == 0                     # label 1 is not applied
        assert ref.fill_holes_rule(ids, None, 1)[3, 0, 10, 10, 60] == 2 and want[3, 0, 10, 10, 60] == 0
        one = pkg.FillHoles()(x[0])
        assert one.shape == x[0].shape and np.array_equal(one.cpu().numpy(), want[0])
    assert gd.check() > 0


def test_fill_holes_transform_random(pkg, dev):
    rng = np.random.default_rng(12)
    z, y, xx = np.meshgrid(np.arange(9), np.arange(17), np.arange(67), indexing="ij")
    ids = (1 + (z // 5 + y // 6 + xx // 9) % 3).astype(np.float32)[None, None].repeat(2, 0)      # blocks of labels 1, 2, 3
    ids[rng.random(ids.shape) < 0.08] = 0
    x = torch.from_numpy(ids).to(dev)
    with Guard(dev) as gd:
        for connectivity in (None, 1, 2):
            for applied in (None, [1, 3]):
                want = ref.fill_holes_rule(ids, applied, connectivity)
                assert 0 < (want != ids).sum() < (ids == 0).sum()
                assert np.array_equal(pkg.FillHoles(applied, connectivity)(x).cpu().numpy(), want)
    assert gd.check() > 0


# ---------------------------------------------------------------------------------------------------- capture, limits
def test_graph_capture(pkg, dev):
    """closing then hole filling, captured once and replayed on other data: no host synchronisation, no per-call state"""
    a, b = (torch.from_numpy(rand_mask((1, 2, 17, 9, 130), d, 13)).float().to(dev) for d in (0.3, 0.4))
    run = lambda t: pkg.binary_fill_holes(pkg.binary_closing(t))
    eager_a, eager_b = run(a), run(b)
    assert not torch.equal(eager_a, eager_b)
    static = a.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static)                                              # warm-up: library load, allocator
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = run(static)
    for src, eager in ((b, eager_b), (a, eager_a)):
        static.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    closed = ref.closing(b.cpu().numpy())
    want = ref.fill_holes(closed)
    assert np.array_equal(eager_b.cpu().numpy(), want) and b.sum().item() < closed.sum() < want.sum() < want.size


def test_limits(pkg, dev):
    with pytest.raises(NotImplementedError):
        pkg.binary_dilation(torch.zeros(1, 17, 2, 2, 2, device=dev))
    with pytest.raises(NotImplementedError):
        pkg.binary_closing(torch.zeros(1, 1, 1, 1, 1025, dtype=torch.uint8, device=dev))
    with pytest.raises(NotImplementedError):
        pkg.binary_fill_holes(torch.zeros(1, 1, 1025, 1, 1, dtype=torch.bool, device=dev))
    with pytest.raises(NotImplementedError):
        pkg.FillHoles()(torch.zeros(1, 1, 1, 1025, 1, device=dev))
    assert pkg._capi.load().unetr_morph_workspace_bytes(1025, 1, 1, 1) == 0
