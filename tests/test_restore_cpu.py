"""Host side of the way back to a scan's own voxel grid (preprocess.Geometry / restore_native, VolumeCache.geometry) and the
float64 restatement tests/restore_ref.py itself.  No GPU: the geometry record is numpy, and every argument error of
restore_native is raised before anything touches a device."""
import numpy as np
import pytest
import torch

import preprocess_ref as R
import restore_ref as RR

ORIGIN = (-12.5, 7.25, 3.0)
SHAPE = (11, 13, 9)


@pytest.mark.parametrize("angle", [0.0, 0.04])
def test_inverse_matrix_inverts_the_forward_matrix(pkg, angle):
    for A in R.signed_permutation_affines((0.8, 0.8, 2.5), ORIGIN, angle):
        g = pkg.preprocess.geometry(SHAPE, A)
        out_shape, mat, new_affine = pkg.preprocess.plan(SHAPE, A)
        assert g.full_shape == out_shape == g.crop_shape and g.crop_origin == (0, 0, 0) and g.native_shape == SHAPE
        assert np.array_equal(g.forward[:3], mat) and np.array_equal(g.forward[3], [0, 0, 0, 1])
        assert np.array_equal(g.oriented_affine, new_affine) and np.array_equal(g.affine, A)
        Minv = g.inverse_matrix()
        assert Minv.shape == (3, 4) and Minv.dtype == np.float64
        assert np.abs(Minv @ g.forward - np.eye(4)[:3]).max() <= 1e-9
        assert np.abs(g.forward[:3] @ RR.as4x4(Minv) - np.eye(4)[:3]).max() <= 1e-9


def test_copy_rule_gives_an_all_integer_inverse(pkg):
    A = np.diag([-1.0, -1.0, 1.0, 1.0])                     # 1 mm LPS
    A[:3, 3] = ORIGIN
    g = pkg.preprocess.geometry(SHAPE, A)
    Minv = g.inverse_matrix()
    assert np.array_equal(Minv, np.rint(Minv))
    assert np.array_equal(Minv, [[-1, 0, 0, SHAPE[0] - 1], [0, -1, 0, SHAPE[1] - 1], [0, 0, 1, 0]])
    # within 1e-3 of 1 mm: MONAI copies forward, so the scan is copied back
    B = A.copy()
    B[:3, :3] *= 1.0004
    gb = pkg.preprocess.geometry(SHAPE, B)
    assert np.array_equal(gb.forward, g.forward) and np.array_equal(gb.inverse_matrix(), Minv)
    for A48 in R.signed_permutation_affines((1.0, 1.0, 1.0), ORIGIN, 0.0):
        m = pkg.preprocess.geometry(SHAPE, A48).inverse_matrix()
        assert np.array_equal(m, np.rint(m))


def test_cropped_shifts_only_the_box(pkg):
    A = R.signed_permutation_affines((0.8, 0.8, 2.5), ORIGIN, 0.04)[17]
    g = pkg.preprocess.geometry(SHAPE, A, (1.0, 1.0, 1.0), "RAS")
    c = g.cropped((1, 2, 3), (4, 5, 6))
    assert c.crop_origin == (1, 2, 3) and c.crop_shape == (4, 5, 6)
    assert g.crop_origin == (0, 0, 0) and g.crop_shape == g.full_shape                # the original is untouched
    for f in ("native_shape", "pixdim", "axcodes", "full_shape"):
        assert getattr(c, f) == getattr(g, f)
    for f in ("affine", "forward", "oriented_affine"):
        assert np.array_equal(getattr(c, f), getattr(g, f))
    assert np.array_equal(c.inverse_matrix(), g.inverse_matrix())
    with pytest.raises(Exception):
        c.crop_origin = (0, 0, 0)                                                     # immutable
    with pytest.raises(ValueError):
        c.forward[0, 0] = 2.0
    with pytest.raises(ValueError, match="inside the grid"):
        g.cropped((0, 0, 0), (g.full_shape[0] + 1, 1, 1))
    with pytest.raises(ValueError, match="inside the grid"):
        g.cropped((-1, 0, 0), (1, 1, 1))


def test_restore_native_argument_errors(pkg):
    A = np.diag([0.8, 0.8, 2.5, 1.0])
    g = pkg.preprocess.geometry((10, 10, 4), A).cropped((1, 1, 1), (6, 6, 7))
    x = torch.zeros(4, 6, 6, 7)
    rn = pkg.restore_native
    with pytest.raises(ValueError, match="crop shape"):
        rn(torch.zeros(4, 6, 6, 6), g)
    with pytest.raises(ValueError, match="crop shape"):
        rn(torch.zeros(4, *g.full_shape), g)
    with pytest.raises(ValueError, match="channels"):
        rn(torch.zeros(17, 6, 6, 7), g)
    with pytest.raises(ValueError, match="mode='linear'"):
        rn(x, g, mode="nearest", post="argmax")
    with pytest.raises(ValueError, match="mode='linear'"):
        rn(x, g, post="sigmoid")
    with pytest.raises(ValueError, match="4 channels"):
        rn(torch.zeros(3, 6, 6, 7), g, label_converter="brats")
    with pytest.raises(ValueError, match="discrete"):
        rn(x, g, mode="linear", label_converter="brats")
    with pytest.raises(ValueError, match="float32"):
        rn(x.double(), g)
    with pytest.raises(ValueError, match="float32"):
        rn(x.to(torch.uint8), g, mode="linear")
    with pytest.raises(ValueError, match="float32"):
        rn(x.to(torch.int16), g)
    with pytest.raises(ValueError, match="batch"):
        rn(torch.zeros(2, 4, 6, 6, 7), g)
    with pytest.raises(ValueError, match="expected"):
        rn(torch.zeros(6, 6, 7), g)
    with pytest.raises(ValueError, match="mode must"):
        rn(x, g, mode="cubic")
    with pytest.raises(ValueError, match="post must"):
        rn(x, g, mode="linear", post="onehot")
    with pytest.raises(ValueError, match="label_converter"):
        rn(x, g, label_converter="rgb")
    with pytest.raises(ValueError, match="Geometry"):
        rn(x, A)
    # out: shape and dtype of the mode's result
    with pytest.raises(ValueError, match="out"):
        rn(x, g, out=torch.zeros(4, 10, 10, 5))
    with pytest.raises(ValueError, match="out"):
        rn(x, g, out=torch.zeros(4, 10, 10, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="out"):
        rn(x, g, mode="linear", post="argmax", out=torch.zeros(4, 10, 10, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="out"):
        rn(x, g, mode="linear", post="sigmoid", out=torch.zeros(4, 10, 10, 4))
    with pytest.raises(ValueError, match="out"):
        rn(x, g, label_converter="brats", out=torch.zeros(4, 10, 10, 4, dtype=torch.uint8))
    # everything valid but the device: the package's usual refusal, for both accepted ranks and every mode
    for kw in (dict(), dict(mode="linear"), dict(mode="linear", post="argmax"),
               dict(mode="linear", post="sigmoid", label_converter="brats"), dict(out=torch.zeros(4, 10, 10, 4))):
        with pytest.raises(RuntimeError, match="ROCm device.*no CPU fallback"):
            rn(x, g, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rn(x[None], g)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rn(x.to(torch.uint8), g, label_converter="brats", out=torch.zeros(1, 10, 10, 4, dtype=torch.uint8))


def test_exports(pkg):
    assert pkg.Geometry is pkg.preprocess.Geometry and pkg.restore_native is pkg.preprocess.restore_native
    assert {"Geometry", "restore_native"} <= set(pkg.__all__)
    assert callable(pkg.VolumeCache.geometry) and callable(pkg.VolumeCache.restore)


# ---------------------------------------------------------------- the restatement itself
def test_ref_without_crop_is_the_fused_gather_with_the_inverse_matrix(pkg):
    rng = np.random.default_rng(3)
    for A in R.signed_permutation_affines((0.8, 0.8, 2.4), ORIGIN, 0.04)[::5]:
        g = pkg.preprocess.geometry(SHAPE, A)
        x = rng.standard_normal((2, *g.full_shape))
        M4 = RR.as4x4(g.inverse_matrix())
        for mode, fmode in (("nearest", "nearest"), ("linear", "bilinear")):
            a = RR.restore(x, M4, SHAPE, g.full_shape, (0, 0, 0), mode)
            assert np.abs(a - R.fused_gather(x, M4, SHAPE, fmode)).max() <= 1e-12
        assert RR.inside_mask(M4, SHAPE, g.full_shape, (0, 0, 0), g.full_shape).all()


def test_ref_crop_is_zero_padding_then_nearest_and_taps_clamped_into_the_box():
    """nearest: exactly CropForegroundd.inverse's zero padding followed by the pick on the full grid; linear: equal to the
    zero-padded interpolation wherever all eight taps lie inside the box, and inside the box's value range on its shell"""
    rng = np.random.default_rng(4)
    full, o, c, native = (12, 10, 9), (2, 1, 3), (7, 6, 4), (9, 8, 20)
    M4 = np.array([[1.31, 0, 0, 0.2], [0, 1.27, 0, -0.1], [0, 0, 0.43, 0.3], [0, 0, 0, 1]])
    x = rng.random((3, *c)) + 1.0
    padded = np.zeros((3, *full))
    padded[:, o[0]:o[0] + c[0], o[1]:o[1] + c[1], o[2]:o[2] + c[2]] = x
    assert np.array_equal(RR.restore(x, M4, native, full, o, "nearest"), R.fused_gather(padded, M4, native, "nearest"))
    lin, pad_lin = RR.restore(x, M4, native, full, o, "linear"), R.fused_gather(padded, M4, native, "bilinear")
    s = RR.coords(M4, native, full)
    f = np.floor(s)
    interior = ((f >= np.array(o)) & (f + 1 <= np.array(o) + np.array(c) - 1)).all(1).reshape(native)
    inside = RR.inside_mask(M4, native, full, o, c).reshape(native)
    assert interior.any() and (inside & ~interior).any() and (~inside).any()
    assert np.abs(lin - pad_lin)[:, interior].max() <= 1e-12
    assert (lin[:, ~inside] == 0).all()
    shell = lin[:, inside & ~interior]
    assert shell.min() >= 1.0 and shell.max() <= 2.0            # a blend of box voxels only: no made-up zero leaks in
    assert (pad_lin[:, inside & ~interior] < 1.0).any()         # whereas zero-pad-then-interpolate does blend zeros in


@pytest.mark.parametrize("spacing", [(1.25, 1.3, 2.5), (1.5, 1.5, 5.0), (1.1, 2.75, 1.9)])
def test_ref_nearest_round_trip_on_a_finer_grid_returns_the_label(pkg, spacing):
    """resampled grid finer than the native one on every axis (pixdim 1 < spacing): the resampled voxel nearest to native voxel
    i reads native voxel i again, because |rint(i k) / k - i| <= 1 / (2 k) < 1 / 2"""
    rng = np.random.default_rng(5)
    for k in spacing:
        i = np.arange(4096.0)
        assert (np.abs(np.rint(i * k) / k - i) < 0.5).all()
    shape = (9, 7, 6)
    affines = R.signed_permutation_affines(spacing, ORIGIN, 0.0)[::3] + R.signed_permutation_affines(spacing, ORIGIN, 0.04)[1::7]
    for n, A in enumerate(affines):
        g = pkg.preprocess.geometry(shape, A)
        assert all(f >= s for f, s in zip(sorted(g.full_shape), sorted(shape)))
        lab = rng.integers(0, 200, (1, *shape))
        fwd = R.fused_gather(lab, g.forward, g.full_shape, "nearest")
        back = RR.restore(fwd, g.inverse_matrix(), shape, g.full_shape, (0, 0, 0), "nearest")
        tie = RR.ties(g.inverse_matrix(), shape, g.full_shape).reshape(shape)
        assert np.array_equal(back[0][~tie], lab[0][~tie].astype(np.float64)), f"case {n}"
        assert (~tie).mean() > 0.25                   # spacing 2.5: every odd index is a tie on that axis


def test_ref_brats_rule_and_argmax():
    ch = np.zeros((4, 1, 1, 6), dtype=bool)
    ch[2, ..., 1:] = True            # WT
    ch[1, ..., 3:] = True            # TC inside WT
    ch[3, ..., 5:] = True            # ET inside TC
    ch[0, ..., 0] = True
    assert RR.brats_label(ch).tolist() == [[[[0, 1, 1, 2, 2, 3]]]]
    v = np.array([[1.0, 2.0, 3.0], [1.0, 5.0, 3.0], [0.0, 5.0, 3.0]]).reshape(3, 1, 1, 3)
    assert RR.argmax_first(v).tolist() == [[[[0, 1, 0]]]]
    assert RR.top_two_gap(v).tolist() == [[[0.0, 0.0, 0.0]]]


def test_ref_equals_the_library_route_backwards(pkg):
    """Spacingd.inverse as the library composes it -- to_norm_affine + affine_grid + grid_sample (border) with the inverse
    transform, here with the Orientation folded into the same affine -- against the fused formula, in float64"""
    import torch.nn.functional as F
    rng = np.random.default_rng(8)
    for A in R.signed_permutation_affines((0.8, 0.8, 2.4), ORIGIN, 0.04)[::7]:
        g = pkg.preprocess.geometry(SHAPE, A)
        x = torch.as_tensor(rng.standard_normal((2, *g.full_shape)))
        M4 = RR.as4x4(g.inverse_matrix())
        theta = R.to_norm_affine_matrix(g.full_shape) @ M4 @ np.linalg.inv(R.to_norm_affine_matrix(SHAPE))
        rev = [2, 1, 0, 3]
        grid = F.affine_grid(torch.as_tensor(theta[rev][:, rev][:3])[None], [1, 2, *SHAPE], align_corners=False)
        for mode, lib in (("linear", "bilinear"), ("nearest", "nearest")):
            want = F.grid_sample(x[None], grid, mode=lib, padding_mode="border", align_corners=False)[0].numpy()
            got = RR.restore(x.numpy(), M4, SHAPE, g.full_shape, (0, 0, 0), mode)
            assert np.abs(got - want).max() <= (1e-9 if mode == "linear" else 0)
