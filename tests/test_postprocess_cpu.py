"""Connected-component post-processing without a GPU: the two CPU references of tests/postprocess_ref.py agree with each other
(so the GPU tests compare against a labelling that was itself checked), and the public names validate their arguments."""
import numpy as np
import pytest
import torch

import postprocess_ref as R


def _tiny_cases():
    """(name, class-id map [1,1,D,H,W], connectivity): seeded random multi-class maps plus hand-made ties"""
    cases = []
    rng = np.random.default_rng(2024)
    shapes = [(3, 4, 5), (1, 6, 7), (4, 3, 3), (2, 5, 6)]
    for i in range(36):
        shape = shapes[i % len(shapes)]
        conn = i % 3 + 1
        nclass = 1 + i % 3
        density = (0.3, 0.5, 0.7)[(i // 3) % 3]
        m = (rng.random(shape) < density) * rng.integers(1, nclass + 1, shape)
        cases.append((f"random{i}", m[None, None].astype(np.float32), conn))
    tie = np.zeros((1, 1, 2, 3, 9), np.float32)
    tie[0, 0, 0, 0, 0:2] = 1          # three components of two voxels each: the raster-first one wins
    tie[0, 0, 0, 2, 3:5] = 1
    tie[0, 0, 1, 1, 7:9] = 1
    tie[0, 0, 1, 0, 0:3] = 2          # class 2: sizes 3, 3
    tie[0, 0, 1, 2, 0:3] = 2
    for conn in (1, 2, 3):
        cases.append((f"ties{conn}", tie, conn))
    diag = np.zeros((1, 1, 2, 2, 2), np.float32)
    diag[0, 0, 0, 0, 0] = diag[0, 0, 0, 1, 1] = 1      # edge contact
    corner = np.zeros((1, 1, 2, 2, 2), np.float32)
    corner[0, 0, 0, 0, 0] = corner[0, 0, 1, 1, 1] = 1  # corner contact
    for conn in (1, 2, 3):
        cases.append((f"edge{conn}", diag, conn))
        cases.append((f"corner{conn}", corner, conn))
    return cases


@pytest.mark.parametrize("independent", [True, False])
def test_references_agree(independent):
    cases = _tiny_cases()
    assert len(cases) >= 36
    for name, m, conn in cases:
        a = R.reference(m, conn, None, independent, labeller=R.label_plane_scipy)
        b = R.reference(m, conn, None, independent, labeller=R.label_plane_bfs)
        for u, v, what in zip(a, b, ("out", "labels", "sizes")):
            assert np.array_equal(u, v), (name, what)
        for min_size in (1, 2, 4):
            a = R.reference(m, conn, None, independent, rule=1, min_size=min_size, labeller=R.label_plane_scipy)[0]
            b = R.reference(m, conn, None, independent, rule=1, min_size=min_size, labeller=R.label_plane_bfs)[0]
            assert np.array_equal(a, b), (name, min_size)


def test_reference_semantics_by_hand():
    cases = {name: (m, conn) for name, m, conn in _tiny_cases()}
    m, _ = cases["ties1"]
    out, labels, sizes = R.reference(m, 1)
    assert labels[0, 0, 0, 0, 0] == 1 and labels[0, 0, 0, 2, 3] == 2 * 9 + 3 + 1
    assert sizes[0, 0, 0, 0, 1] == 2 and sizes[0, 0, 1, 2, 2] == 3
    assert out[0, 0, 0, 0, 0] == 1 and out[0, 0, 0, 2, 3] == 0 and out[0, 0, 1, 1, 7] == 0      # raster-first of the tie
    assert out[0, 0, 1, 0, 1] == 2 and out[0, 0, 1, 2, 1] == 0
    for conn, n_edge, n_corner in ((1, 2, 2), (2, 1, 2), (3, 1, 1)):
        assert len(np.unique(R.reference(cases[f"edge{conn}"][0], conn)[1])) - 1 == n_edge
        assert len(np.unique(R.reference(cases[f"corner{conn}"][0], conn)[1])) - 1 == n_corner
    # one-hot, not independent: one mask over the applied channels, the unapplied channel passes through
    x = np.zeros((1, 3, 1, 1, 7), np.float32)
    x[0, 0, 0, 0, :] = 1
    x[0, 1, 0, 0, 0:2] = 1
    x[0, 2, 0, 0, 2:3] = 1
    x[0, 2, 0, 0, 5:6] = 1
    out, labels, _ = R.reference(x, 1, [1, 2], independent=False)
    assert np.array_equal(out[0, 0], x[0, 0]) and out[0, 2, 0, 0, 2] == 1 and out[0, 2, 0, 0, 5] == 0
    assert labels[0, 1, 0, 0, 1] == 1 and labels[0, 2, 0, 0, 2] == 1 and labels[0, 2, 0, 0, 5] == 6 and not labels[0, 0].any()


def test_public_names_and_argument_checks(pkg):
    P = pkg.postprocess
    for name in ("KeepLargestConnectedComponent", "connected_components", "remove_small_components"):
        assert getattr(pkg, name) is getattr(P, name) and name in pkg.__all__
    m = torch.zeros(1, 1, 2, 3, 4)
    for bad in (0, 4, 1.5, "full"):
        with pytest.raises(ValueError, match="connectivity"):
            pkg.connected_components(m, connectivity=bad)
        with pytest.raises(ValueError, match="connectivity"):
            pkg.KeepLargestConnectedComponent([1], connectivity=bad)
    with pytest.raises(ValueError, match="background"):
        pkg.KeepLargestConnectedComponent([0])(m)
    with pytest.raises(ValueError, match="background"):
        pkg.connected_components(torch.zeros(1, 3, 2, 3, 4), applied_labels=[0, 1], from_logits=True)
    with pytest.raises(NotImplementedError):
        pkg.connected_components(m, applied_labels=[32])
    with pytest.raises(ValueError):
        pkg.connected_components(torch.zeros(1, 3, 2, 3, 4), applied_labels=[3])
    with pytest.raises(NotImplementedError, match="16"):
        pkg.connected_components(torch.zeros(1, 17, 1, 1, 2))
    with pytest.raises(NotImplementedError, match="1024"):
        pkg.KeepLargestConnectedComponent([1])(torch.zeros(1, 1, 1, 1, 1025))
    with pytest.raises(ValueError):
        pkg.connected_components(torch.zeros(2, 3, 4))
    with pytest.raises(ValueError, match="min_size"):
        pkg.remove_small_components(m, -1)


def test_cpu_tensors_raise(pkg):
    m = torch.ones(1, 1, 2, 3, 4)
    with pytest.raises(RuntimeError, match="ROCm device"):
        pkg.connected_components(m)
    with pytest.raises(RuntimeError, match="ROCm device"):
        pkg.KeepLargestConnectedComponent([1])([m[0], m[0]])
    with pytest.raises(RuntimeError, match="ROCm device"):
        pkg.remove_small_components(m, 2)


def test_workspace_bytes(pkg):
    lib = pkg._capi.load()
    D, H, W = 24, 24, 70
    sizes = [lib.unetr_ccl_workspace_bytes(D, H, W, g) for g in range(0, 6)]
    assert sizes[0] == 0 and all(b > a for a, b in zip(sizes, sizes[1:]))
    assert sizes[1] >= 9 * D * H * W and sizes[5] - sizes[4] <= 9 * D * H * W + 5 * 256
    assert lib.unetr_ccl_workspace_bytes(1, 1, 1025, 1) == 0 and lib.unetr_ccl_workspace_bytes(0, 4, 4, 1) == 0
