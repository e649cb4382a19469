"""The references of tests/distance_ref.py against scipy and against values computed by hand, the host side of the distance-map
losses (constructor validation, exports), and the band condition of the Hausdorff-DT inputs.  No GPU."""
import numpy as np
import pytest
import torch

from distance_ref import (BAND, EDT_SHAPES, LOSS_CASES, MASK_KINDS, SPACING, band_count, boundary_loss_ref, edt_ref, field_ref,
                          hausdorff_dt_loss_ref, loss_inputs, make_mask)


@pytest.mark.parametrize("shape", EDT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edt_ref_equals_scipy(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    checked = 0
    for kind in MASK_KINDS:
        m = make_mask(kind, shape)
        if m.all():                      # scipy leaves arbitrary values there; the reference says +inf
            assert torch.isinf(edt_ref(m)).all()
            continue
        ref2 = edt_ref(m, squared=True)
        assert ref2.dtype == torch.int64
        sp = ndi.distance_transform_edt(m.numpy())
        # scipy returns sqrt of the exact integer: squaring and rounding recovers it
        assert np.array_equal(np.rint(sp * sp).astype(np.int64), ref2.numpy()), kind
        assert np.array_equal(sp, np.sqrt(ref2.numpy().astype(np.float64))), kind
        s32 = [float(np.float32(v)) for v in SPACING]
        sps = ndi.distance_transform_edt(m.numpy(), sampling=s32)
        np.testing.assert_allclose(edt_ref(m, SPACING).numpy(), sps, rtol=1e-12, atol=0, err_msg=kind)
        checked += 1
    assert checked >= 4


def test_field_ref_degenerate_objects_are_zero():
    for obj in (torch.zeros(3, 4, 5, dtype=torch.bool), torch.ones(3, 4, 5, dtype=torch.bool)):
        for unsigned in (False, True):
            f = field_ref(obj, None, unsigned)
            assert f.shape == obj.shape and not f.any()


# The example of both hand computations: B = 1, C = 2, spatial (1, 1, 4).  Class ids 0 0 1 1; logits with z1 - z0 = -ln3, ln3, -ln3, ln3,
# so p1 = 1/4, 3/4, 1/4, 3/4 and p0 = 1 - p1.
def _example():
    z = torch.zeros(1, 2, 1, 1, 4, dtype=torch.float64)
    z[0, 1, 0, 0] = torch.tensor([-1.0, 1.0, -1.0, 1.0], dtype=torch.float64) * np.log(3.0)
    return z, torch.tensor([0.0, 0.0, 1.0, 1.0]).view(1, 1, 1, 1, 4)


def test_boundary_loss_ref_by_hand():
    """Channel 1 (object = voxels 2, 3): d_fg = 2, 1 outside, -(d_bg - 1) = -(1 - 1), -(2 - 1) = 0, -1 inside: phi_1 = 2, 1, 0, -1.
    sum p1 phi_1 = 0.5 + 0.75 + 0 - 0.75 = 0.5; mean over the 4 voxels = 0.125.
    Channel 0 (object = voxels 0, 1): phi_0 = -1, 0, 1, 2; sum p0 phi_0 = -0.75 + 0 + 0.75 + 0.5 = 0.5; with the background the mean
    over 8 = 0.125 again."""
    z, y = _example()
    assert field_ref(y[0, 0] == 1).flatten().tolist() == [2.0, 1.0, 0.0, -1.0]
    assert field_ref(y[0, 0] == 0).flatten().tolist() == [-1.0, 0.0, 1.0, 2.0]
    assert abs(float(boundary_loss_ref(z, y)) - 0.125) < 1e-15
    assert abs(float(boundary_loss_ref(z, y, include_background=True)) - 0.125) < 1e-15
    assert abs(float(boundary_loss_ref(z, y, weight=0.5)) - 0.0625) < 1e-15
    # 2 mm voxels double the distances and the offset u: phi_1 = 4, 2, 0, -2, and the loss
    assert abs(float(boundary_loss_ref(z, y, spacing=(2.0, 2.0, 2.0))) - 0.25) < 1e-15
    # 2 mm along x only: u = the smallest spacing = 1, phi_1 = 4, 2, -(2 - 1), -(4 - 1); sum p1 phi_1 = 1 + 1.5 - 0.25 - 2.25 = 0
    assert abs(float(boundary_loss_ref(z, y, spacing=(1.0, 1.0, 2.0)))) < 1e-15
    assert field_ref(y[0, 0] == 1, (2.0, 2.0, 2.0)).flatten().tolist() == [4.0, 2.0, 0.0, -2.0]


def test_hausdorff_dt_loss_ref_by_hand():
    """Channel 1, alpha = 2.  Target 0 0 1 1: F_G = 2, 1, 1, 2, squared 4, 1, 1, 4.  Prediction p1 > 0.5 = 0 1 0 1: every voxel has the
    other value next to it, F_P = 1, 1, 1, 1.  F_P^2 + F_G^2 = 5, 2, 2, 5.  (p1 - g1)^2 = 1/16, 9/16, 9/16, 1/16.
    sum = (5 + 18 + 18 + 5) / 16 = 2.875; mean over the 4 voxels = 0.71875.  alpha = 1: 3, 2, 2, 3 -> (3 + 18 + 18 + 3) / 16 / 4 = 0.65625."""
    z, y = _example()
    assert field_ref(y[0, 0] == 1, None, True).flatten().tolist() == [2.0, 1.0, 1.0, 2.0]
    assert abs(float(hausdorff_dt_loss_ref(z, y)) - 0.71875) < 1e-15
    assert abs(float(hausdorff_dt_loss_ref(z, y, alpha=1.0)) - 0.65625) < 1e-15
    # channel 0 mirrors channel 1 (p0 - g0 = -(p1 - g1), the same boundaries): the mean over both channels is the same number
    assert abs(float(hausdorff_dt_loss_ref(z, y, include_background=True)) - 0.71875) < 1e-15
    # F_P carries no gradient: the gradient is that of (p - g)^2 with the field held constant
    zz = z.clone().requires_grad_(True)
    hausdorff_dt_loss_ref(zz, y).backward()
    p1 = torch.tensor([0.25, 0.75, 0.25, 0.75], dtype=torch.float64)
    g1 = torch.tensor([0.0, 0.0, 1.0, 1.0], dtype=torch.float64)
    want = 2 * (p1 - g1) * torch.tensor([5.0, 2.0, 2.0, 5.0], dtype=torch.float64) * p1 * (1 - p1) / 4
    assert torch.allclose(zz.grad[0, 1, 0, 0], want, rtol=1e-14, atol=0)


def test_exports(pkg):
    for name in ("distance_transform_edt", "signed_distance_map", "BoundaryLoss", "HausdorffDTLoss"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert hasattr(pkg.distance, "prediction_distance_map")


@pytest.mark.parametrize("name", ["BoundaryLoss", "HausdorffDTLoss"])
def test_constructor_validation(pkg, name):
    cls = getattr(pkg, name)
    for kw in (dict(to_onehot_y=True, softmax=True), dict(to_onehot_y=False, sigmoid=True)):
        crit = cls(**kw)
        assert crit.weight.dtype == torch.float32 and crit.weight.numel() == 1 and float(crit.weight) == 1.0
        assert crit.cfg["include_background"] == 0
    with pytest.raises(ValueError, match="exclude each other"):
        cls(softmax=True, sigmoid=True)
    for kw in (dict(), dict(to_onehot_y=True), dict(softmax=True), dict(to_onehot_y=True, sigmoid=True), dict(sigmoid=False)):
        with pytest.raises(NotImplementedError, match="to_onehot_y=True with softmax=True"):
            cls(**kw)
    for red in ("sum", "none"):
        with pytest.raises(NotImplementedError, match="reduction"):
            cls(to_onehot_y=True, softmax=True, reduction=red)
    with pytest.raises(TypeError):
        cls(to_onehot_y=True, softmax=True, ignore_index=255)
    for sp in ((1.0, 2.0), (1.0, 0.0, 1.0), (1.0, -1.0, 1.0)):
        with pytest.raises(ValueError, match="spacing"):
            cls(to_onehot_y=True, softmax=True, spacing=sp)
    crit = cls(to_onehot_y=True, softmax=True, weight=0.37, spacing=(3.0, 0.7, 1.5))
    assert float(crit.weight) == float(torch.tensor(0.37)) and crit.spacing == (3.0, 0.7, 1.5)
    crit.set_weight(0.25)
    assert float(crit.weight) == 0.25
    if name == "HausdorffDTLoss":
        assert cls(to_onehot_y=True, softmax=True).alpha == 2.0
        with pytest.raises(ValueError, match="alpha"):
            cls(alpha=0.0, to_onehot_y=True, softmax=True)


def test_no_cpu_fallback(pkg):
    with pytest.raises(RuntimeError, match="ROCm device"):
        pkg.distance_transform_edt(torch.zeros(4, 4, 4))
    with pytest.raises(RuntimeError, match="ROCm device"):
        pkg.signed_distance_map(torch.zeros(1, 1, 4, 4, 4), num_classes=2)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="ROCm device"):
            pkg.BoundaryLoss(to_onehot_y=True, softmax=True)(torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4))


@pytest.mark.parametrize("case", [c for c in LOSS_CASES if c[1] == "hausdorff"], ids=lambda c: c[0])
def test_band_condition_of_the_hausdorff_inputs(case):
    """no probability of a Hausdorff-DT case lies within BAND of the 0.5 threshold (float64 from the float32 logits)"""
    _, _, shape, mode, label, logit, _ = case
    logits, target, before = loss_inputs(shape, mode, label, logit)
    assert logits.dtype == torch.float32
    p = torch.sigmoid(logits.double()) if mode == "ml" else torch.softmax(logits.double(), 1)
    assert float((p - 0.5).abs().min()) >= BAND
    assert band_count(logits, mode == "ml") == 0


def test_band_step_is_needed():
    """the seeded logits do hold probabilities inside the band before the step moves them"""
    counts = {c[0]: loss_inputs(c[2], c[3], c[4], c[5])[2] for c in LOSS_CASES if c[1] == "hausdorff"}
    print(counts)
    assert sum(counts.values()) > 0
