"""CPU checks of the resampling / reorientation host logic: preprocess.plan against the restatement of tests/preprocess_ref.py
for all 48 signed axis permutations (axis-aligned and oblique) and the identity shortcut, the restatement's library route
(affine_grid + grid_sample, then flip / transpose) against the fused formula the kernel implements, and the public signatures.
test_library_route_equals_fused_formula and test_brats_converter_commutes_with_nearest check the restatement itself (they do not
touch the package): they tie the formula the kernel implements to the library's composition."""
import inspect

import numpy as np
import pytest
import torch

import preprocess_ref as R

SPACING, ORIGIN, SHAPE = (0.79, 0.83, 2.3), (-12.5, 7.25, 3.0), (20, 18, 9)
RAS = np.array([[0, 1], [1, 1], [2, 1]], dtype=np.float64)


def _volume(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.random((1, *shape)) * 400 - 200, rng.integers(0, 4, (1, *shape)).astype(np.float64)


@pytest.mark.parametrize("angle", [0.0, 0.04])
def test_plan_equals_restatement_all_orientations(pkg, angle):
    for A in R.signed_permutation_affines(SPACING, ORIGIN, angle):
        x, _ = _volume(SHAPE, 0)
        y, aff, TM = R.library_route(x, A, (1, 1, 1), "RAS", "nearest")
        out_shape, mat, new_affine = pkg.preprocess.plan(SHAPE, A, (1.0, 1.0, 1.0), "RAS")
        assert out_shape == y.shape[1:]
        assert mat.shape == (3, 4) and mat.dtype == np.float64
        assert np.abs(mat - TM[:3]).max() <= 1e-12 and np.abs(new_affine - aff).max() <= 1e-12
        assert np.array_equal(R.io_orientation(new_affine), RAS)


def test_plan_identity_shortcut(pkg):
    """1 mm data (BraTS): Spacing copies, so the matrix is the exact integer flip / transpose of Orientation alone"""
    for A in R.signed_permutation_affines((1.0, 1.0, 1.0), ORIGIN, 0.0) + R.signed_permutation_affines((1.0, 1.0003, 0.9998), ORIGIN, 0.0):
        x, _ = _volume(SHAPE, 1)
        y, aff, TM = R.library_route(x, A, (1, 1, 1), "RAS", "bilinear")
        out_shape, mat, new_affine = pkg.preprocess.plan(SHAPE, A)
        assert out_shape == y.shape[1:] and sorted(out_shape) == sorted(SHAPE)
        assert np.array_equal(mat, np.rint(mat)) and np.array_equal(mat, TM[:3])
        assert np.abs(new_affine - aff).max() <= 1e-12
        assert np.array_equal(R.io_orientation(new_affine), RAS)
        assert np.array_equal(R.fused_gather(x, np.vstack([mat, [0, 0, 0, 1]]), out_shape, "bilinear"), y)


@pytest.mark.parametrize("axcodes", ["LPS", "ASL", "SRP"])
def test_plan_other_axcodes(pkg, axcodes):
    want = R.axcodes2ornt(axcodes)
    for A in R.signed_permutation_affines(SPACING, ORIGIN, 0.04)[::5]:
        x, _ = _volume(SHAPE, 2)
        y, aff, TM = R.library_route(x, A, (1.5, 1.0, 2.0), axcodes, "nearest")
        out_shape, mat, new_affine = pkg.preprocess.plan(SHAPE, A, (1.5, 1.0, 2.0), axcodes)
        assert out_shape == y.shape[1:]
        assert np.abs(mat - TM[:3]).max() <= 1e-12 and np.abs(new_affine - aff).max() <= 1e-12
        assert np.array_equal(R.ornt_transform(R.io_orientation(new_affine), want), RAS)


@pytest.mark.parametrize("angle", [0.0, 0.04])
def test_library_route_equals_fused_formula(angle):
    """ties the formula of the kernel to the library's composition: bilinear to 1e-9, nearest exactly (no ties in these inputs)"""
    worst = 0.0
    for n, A in enumerate(R.signed_permutation_affines(SPACING, ORIGIN, angle)):
        x, lab = _volume(SHAPE, n)
        y, _, TM = R.library_route(x, A, (1, 1, 1), "RAS", "bilinear")
        yl, _, _ = R.library_route(lab, A, (1, 1, 1), "RAS", "nearest")
        assert R.tie_mask(TM, y.shape[1:], SHAPE).mean() == 0
        worst = max(worst, np.abs(R.fused_gather(x, TM, y.shape[1:], "bilinear") - y).max())
        assert np.array_equal(R.fused_gather(lab, TM, y.shape[1:], "nearest"), yl)
    assert worst <= 1e-9, worst


def test_brats_converter_commutes_with_nearest():
    A = R.signed_permutation_affines(SPACING, ORIGIN, 0.04)[13]
    _, lab = _volume(SHAPE, 3)
    per_channel, _, TM = R.library_route(R.brats_channels(lab[0]), A, (1, 1, 1), "RAS", "nearest")
    picked = R.fused_gather(lab, TM, per_channel.shape[1:], "nearest")
    assert np.array_equal(R.brats_channels(picked[0]), per_channel)


def test_plan_rejects_bad_arguments(pkg):
    A = np.diag([0.8, 0.8, 2.5, 1.0])
    with pytest.raises(ValueError, match="4x4"):
        pkg.preprocess.plan(SHAPE, np.eye(3))
    with pytest.raises(ValueError, match="pixdim"):
        pkg.preprocess.plan(SHAPE, A, (1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="pixdim"):
        pkg.preprocess.plan(SHAPE, A, (1.0, 1.0))
    S = A.copy()
    S[:, 1] = S[:, 0]
    with pytest.raises(ValueError, match="singular"):
        pkg.preprocess.plan(SHAPE, S)
    with pytest.raises(ValueError, match="axcodes"):
        pkg.preprocess.plan(SHAPE, A, axcodes="RAR")
    with pytest.raises(ValueError, match="spatial extents"):
        pkg.preprocess.plan((4, 4), A)


def test_public_signatures(pkg):
    assert pkg.resample_orient is pkg.preprocess.resample_orient and "resample_orient" in pkg.__all__
    assert list(inspect.signature(pkg.resample_orient).parameters) == ["image", "label", "affine", "pixdim", "axcodes",
                                                                       "label_converter"]
    p = inspect.signature(pkg.VolumeCache.add_raw).parameters
    assert list(p) == ["self", "image", "label", "affine", "pixdim", "axcodes", "label_converter", "scale_range", "crop_foreground"]
    assert p["pixdim"].default == (1.0, 1.0, 1.0) and p["axcodes"].default == "RAS" and p["label_converter"].default is None
    assert p["scale_range"].default is None and p["crop_foreground"].default is False
    assert list(inspect.signature(pkg.preprocess.plan).parameters) == ["shape", "affine", "pixdim", "axcodes"]
    assert callable(pkg.VolumeCache.affine)
    assert "unetr_resample_orient" in pkg._capi.EXPORTED_SYMBOLS and pkg._capi.ABI_VERSION == 21


def test_cpu_tensors_have_no_fallback(pkg):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.resample_orient(torch.zeros(1, 4, 4, 4), None, np.eye(4))
    with pytest.raises(ValueError, match="label_converter"):
        pkg.resample_orient(torch.zeros(1, 4, 4, 4), None, np.eye(4), label_converter="rgb")
