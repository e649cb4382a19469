"""GPU connected-component post-processing (csrc/postprocess.hip) against the scipy reference of
tests/postprocess_ref.py.  Every comparison is exact: canonical labels and sizes are integers, the filtered output is compared
bit for bit.  Shapes are the smallest at which the kernels can still go wrong: W odd, crossing the 64-lane segment, several
workgroups, equivalence chains that span them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import postprocess_ref as R

pytestmark = pytest.mark.gpu


def _check(pkg, dev, x, conn, applied, independent=True, from_logits=False):
    """labels, sizes and the keep-largest output of x (numpy [B,C,D,H,W]) against the reference; returns the reference"""
    want_out, want_labels, want_sizes = R.reference(x, conn, applied, independent, from_logits)
    t = torch.from_numpy(x).to(dev)
    labels, sizes = pkg.connected_components(t, conn, applied, independent, from_logits, return_sizes=True)
    assert labels.dtype == torch.int32 and sizes.dtype == torch.int32
    assert np.array_equal(labels.cpu().numpy(), want_labels), "labels"
    assert np.array_equal(sizes.cpu().numpy(), want_sizes), "sizes"
    assert torch.equal(pkg.connected_components(t, conn, applied, independent, from_logits), labels)
    out = pkg.KeepLargestConnectedComponent(applied, independent, conn)(t, from_logits=from_logits)
    assert out.dtype == torch.float32 and out.data_ptr() != t.data_ptr()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want_out.view(np.uint32)), "keep-largest output"
    assert torch.equal(t, torch.from_numpy(x).to(dev)), "the input was modified"
    return want_out, want_labels, want_sizes


def _n_components(labels):
    return len(np.unique(labels)) - int((labels == 0).any())


@pytest.mark.parametrize("shape", [(1, 1, 5, 7, 67), (2, 1, 17, 9, 130), (1, 1, 24, 24, 70)])
@pytest.mark.parametrize("conn,density", [(1, 0.30), (2, 0.15), (3, 0.10)])
def test_random_masks_against_scipy(pkg, dev, shape, conn, density):
    rng = np.random.default_rng(shape[4] * 10 + conn)
    x = (rng.random(shape) < density).astype(np.float32)
    _, labels, _ = _check(pkg, dev, x, conn, [1])
    counts = pkg.postprocess.count_components(torch.from_numpy(x).to(dev), conn, [1]).cpu().numpy()
    assert counts.shape == (shape[0], 32)
    for b in range(shape[0]):
        assert counts[b, 1] == _n_components(labels[b]) and counts[b].sum() == counts[b, 1]


def _chain_volume(kind):
    D, H, W = 64, 96, 200
    m = np.zeros((D, H, W), np.float32)
    if kind == "serpentine":           # one path, one voxel thick, through every second row of every second plane
        for zi, z in enumerate(range(0, D, 2)):
            for yi, y in enumerate(range(0, H, 2)):
                m[z, y, :] = 1
                if y + 2 < H:
                    m[z, y + 1, W - 1 if yi % 2 == 0 else 0] = 1
            if z + 2 < D:              # row 94 is traversed right to left, so a plane's path runs (0, 0) -> (94, 0) or back
                m[z + 1, H - 2 if zi % 2 == 0 else 0, 0] = 1
    elif kind == "comb":               # teeth along x that join only at the far end
        m[::2, ::2, :] = 1
        m[:, :, W - 1] = 1
    elif kind == "full":
        m[:] = 1
    return m[None, None]


@pytest.mark.parametrize("conn", [1, 3])
@pytest.mark.parametrize("kind", ["serpentine", "comb", "full", "empty"])
def test_long_equivalence_chains_across_workgroups(pkg, dev, kind, conn):
    x = _chain_volume(kind)
    out, labels, sizes = _check(pkg, dev, x, conn, [1])
    if kind == "empty":
        assert not labels.any() and not out.any()
    else:                              # the inputs are what they claim to be: one component whose first voxel is voxel 0
        assert _n_components(labels) == 1 and labels.max() == 1 and sizes.max() == int(x.sum())
        assert np.array_equal(out, x)


@pytest.mark.parametrize("conn", [1, 2, 3])
def test_connectivity_is_respected(pkg, dev, conn):
    W = 130
    x = np.zeros((4, 1, 3, 4, W), np.float32)
    x[0, 0, 0, 0, 63] = x[0, 0, 0, 1, 64] = 1          # edge contact across the wave-segment boundary
    x[1, 0, 0, 1, 63] = x[1, 0, 1, 2, 64] = 1          # corner contact across it
    x[2, 0, 1, 1, W - 1] = x[2, 0, 1, 2, 0] = 1        # last and first voxels of adjacent rows: adjacent in memory only
    x[3, 0, 0, 3, W - 1] = x[3, 0, 1, 0, 0] = 1        # the same across a plane boundary
    _, labels, _ = _check(pkg, dev, x, conn, [1])
    want = {1: [2, 2, 2, 2], 2: [1, 2, 2, 2], 3: [1, 1, 2, 2]}[conn]
    assert [_n_components(labels[b]) for b in range(4)] == want
    counts = pkg.postprocess.count_components(torch.from_numpy(x).to(dev), conn).cpu().numpy()
    assert counts[:, 1].tolist() == want


@pytest.mark.parametrize("conn", [1, 2, 3])
def test_classes_never_merge(pkg, dev, conn):
    rng = np.random.default_rng(7 + conn)
    x = rng.integers(1, 4, (1, 1, 9, 10, 70)).astype(np.float32)       # no background: different classes touch everywhere
    _, labels, _ = _check(pkg, dev, x, conn, [1, 2, 3], independent=True)
    for lab in np.unique(labels):
        assert len(np.unique(x[labels == lab])) == 1
    out, labels, _ = _check(pkg, dev, x, conn, [1, 2, 3], independent=False)
    assert _n_components(labels) == 1 and np.array_equal(out, x)
    out, labels, _ = _check(pkg, dev, x, conn, [2])
    assert np.array_equal(out[x != 2].view(np.uint32), x[x != 2].view(np.uint32)) and not labels[x != 2].any()
    assert (out[x == 2] == 2).any() and (conn > 1 or (out[x == 2] == 0).any())
    _check(pkg, dev, x, conn, [1, 3], independent=False)


def test_ties_keep_the_raster_first_component(pkg, dev):
    W = 130
    two = np.zeros((1, 1, 4, 8, W), np.float32)
    # A's smallest voxel is the single voxel at the END of row 0; its long run in row 1 starts with a larger provisional label
    two[0, 0, 0, 0, W - 1] = 1
    two[0, 0, 0, 1, :] = 1
    two[0, 0, 2, 0, :] = 1                             # B: the same size, later in raster order
    two[0, 0, 2, 1, 0] = 1
    three = two.copy()
    three[0, 0, 3, 3, :] = 1                           # C
    three[0, 0, 3, 4, 5] = 1
    for x, n in ((two, 2), (three, 3)):
        for conn in (1, 3):
            out, labels, sizes = _check(pkg, dev, x, conn, [1])
            assert _n_components(labels) == n and set(np.unique(sizes)) == {0, W + 1}
            assert out[0, 0, 0].sum() == W + 1 and not out[0, 0, 1:].any() and labels[0, 0, 0, 1, 0] == W


def test_onehot_multilabel_and_logits(pkg, dev, monkeypatch):
    rng = np.random.default_rng(11)
    x = (rng.random((2, 4, 6, 7, 67)) < 0.3).astype(np.float32)       # overlapping channels
    x[0, 2] *= 3.0                                                      # multi-label: any non-zero value is foreground
    for conn in (1, 3):
        _check(pkg, dev, x, conn, [0, 1, 2, 3], independent=True)
        out, labels, _ = _check(pkg, dev, x, conn, [0, 1, 3], independent=True)
        assert np.array_equal(out[:, 2], x[:, 2]) and not labels[:, 2].any()       # the unapplied channel passes through
        out, _, _ = _check(pkg, dev, x, conn, [1, 2, 3], independent=False)
        assert np.array_equal(out[:, 0], x[:, 0])
    # several plane groups under a small workspace budget give the same result
    monkeypatch.setattr(pkg.postprocess, "CCL_PLANE_BUDGET_BYTES", 3 * 9 * 6 * 7 * 67 + 4096)
    _check(pkg, dev, x, 2, [0, 1, 2, 3], independent=True)
    monkeypatch.undo()
    # logits: the first-maximum argmax, then the class-id route
    logits = rng.integers(-2, 3, (2, 4, 6, 7, 67)).astype(np.float32)             # many exact ties between channels
    _check(pkg, dev, logits, 2, [1, 3], from_logits=True)
    _check(pkg, dev, logits, 3, [1, 2, 3], independent=False, from_logits=True)
    t = torch.from_numpy(logits).to(dev)
    klcc = pkg.KeepLargestConnectedComponent([1, 2, 3], connectivity=1)
    ids = t.argmax(dim=1, keepdim=True).float()
    got = klcc(t, from_logits=True)
    assert got.shape == (2, 1, 6, 7, 67) and torch.equal(got, klcc(ids))
    # input forms: a list of decollated items, one [C, D, H, W] item, items of unequal shapes, another dtype
    xt = torch.from_numpy(x).to(dev)
    klcc = pkg.KeepLargestConnectedComponent([1, 2, 3], independent=True, connectivity=2)
    batch = klcc(xt)
    items = klcc(list(xt.unbind(0)))
    assert isinstance(items, list) and len(items) == 2 and items[0].shape == (4, 6, 7, 67)
    assert torch.equal(torch.stack(items), batch) and torch.equal(klcc(xt[1]), batch[1])
    mixed = klcc([xt[0], xt[1, :, :5].contiguous()])
    assert torch.equal(mixed[0], batch[0]) and mixed[1].shape == (4, 5, 7, 67)
    assert torch.equal(mixed[1], klcc(xt[1:2, :, :5].contiguous())[0])
    assert torch.equal(klcc(xt.to(torch.uint8)), batch)


@pytest.mark.parametrize("conn", [1, 2, 3])
def test_remove_small_components_against_reference(pkg, dev, conn):
    rng = np.random.default_rng(23 + conn)
    m = ((rng.random((2, 1, 17, 9, 130)) < 0.25) * rng.integers(1, 3, (2, 1, 17, 9, 130))).astype(np.float32)
    onehot = (rng.random((1, 3, 6, 7, 67)) < 0.3).astype(np.float32)
    largest = int(R.reference(m, conn)[2].max())
    for min_size in (0, 1, 2, 5, largest, largest + 1):
        for x, applied, independent in ((m, None, True), (m, [1, 2], False), (m, [2], True), (onehot, [0, 2], True),
                                        (onehot, None, False)):
            want = R.reference(x, conn, applied, independent, rule=1, min_size=min_size)[0]
            got = pkg.remove_small_components(torch.from_numpy(x).to(dev), min_size, conn, applied, independent)
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), (min_size, applied, independent)
    x = torch.from_numpy(m).to(dev)
    assert torch.equal(pkg.remove_small_components(x, 1, conn), x)
    assert not pkg.remove_small_components(x, largest + 1, conn).any()


def test_results_are_reproducible(pkg, dev):
    rng = np.random.default_rng(5)
    x = torch.from_numpy(((rng.random((1, 1, 24, 24, 70)) < 0.3) * rng.integers(1, 4, (1, 1, 24, 24, 70))).astype(np.float32)).to(dev)
    klcc = pkg.KeepLargestConnectedComponent([1, 2, 3])
    first = (*pkg.connected_components(x, 1, return_sizes=True), klcc(x))
    for _ in range(3):
        again = (*pkg.connected_components(x, 1, return_sizes=True), klcc(x))
        assert all(torch.equal(a, b) for a, b in zip(first, again))


def test_call_is_capturable_in_a_graph(pkg, dev):
    """no host synchronisation: the call is captured on a side stream and replayed on a second input"""
    rng = np.random.default_rng(9)
    a, b = (torch.from_numpy((rng.random((2, 1, 17, 9, 130)) < 0.3).astype(np.float32)).to(dev) for _ in range(2))
    klcc = pkg.KeepLargestConnectedComponent([1], connectivity=1)
    eager = (klcc(b), *pkg.connected_components(b, 1, return_sizes=True))
    static = a.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        klcc(static)                                                   # warm-up: library load, allocator
        pkg.connected_components(static, 1, return_sizes=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = klcc(static)
        labels, sizes = pkg.connected_components(static, 1, return_sizes=True)
    static.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[0]) and torch.equal(labels, eager[1]) and torch.equal(sizes, eager[2])
    assert not torch.equal(out, klcc(a))


def test_composition_with_inferer_and_hausdorff(pkg, dev):
    """klcc(inferer(x, net, post="argmax")) removes a distant island, and the Hausdorff distance drops to the blob's"""
    D, H, W = 40, 48, 44
    x = torch.zeros(1, 1, D, H, W)
    x[0, 0, 8:20, 10:30, 6:24] = 1             # the organ
    x[0, 0, 34:36, 40:43, 38:41] = 1           # a stray island
    truth = torch.zeros(1, 1, D, H, W)
    truth[0, 0, 8:20, 10:30, 6:23] = 1         # ground truth: the organ, one voxel shorter along x
    net = lambda w: torch.cat([0.5 - w, w - 0.5], 1)                  # "paints" class 1 where the input is set
    inferer = pkg.SlidingWindowInferer((32, 32, 32), 2, overlap=0.25)
    ids = inferer(x.to(dev), net, post="argmax")
    assert torch.equal(ids.cpu(), x)
    kept = pkg.KeepLargestConnectedComponent([1])(ids)
    want = x.clone()
    want[0, 0, 34:36, 40:43, 38:41] = 0
    assert torch.equal(kept.cpu(), want)
    onehot = lambda t: F.one_hot(t[:, 0].long(), 2).movedim(-1, 1).float().contiguous()
    hd = pkg.HausdorffDistanceMetric(include_background=False)
    before = hd(onehot(ids), onehot(truth.to(dev))).item()
    after = hd(onehot(kept), onehot(truth.to(dev))).item()
    island = float(np.sqrt((35 - 19) ** 2 + (42 - 29) ** 2 + (40 - 22) ** 2))   # farthest island voxel to the nearest truth voxel
    assert before == pytest.approx(island, abs=1e-12) and after == 1.0
