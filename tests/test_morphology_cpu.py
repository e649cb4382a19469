"""Host side of the morphology module: argument validation, the identities of the scipy reference that the kernels lean on,
and a numpy uint64 model of the bit-packed step that pins the three word formulas of csrc/morphology.hip against scipy."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import morphology_ref as ref

NAMES = ["binary_dilation", "binary_erosion", "binary_opening", "binary_closing", "binary_contour", "binary_fill_holes", "FillHoles"]


def rand_mask(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------- validation
def test_argument_validation(pkg):
    x = torch.zeros(1, 1, 4, 4, 4)
    for fn in (pkg.binary_dilation, pkg.binary_erosion, pkg.binary_opening, pkg.binary_closing):
        with pytest.raises(ValueError, match="repeat until nothing changes"):
            fn(x, iterations=0)
        with pytest.raises(ValueError, match="iterations"):
            fn(x, iterations=1.5)
    for fn in (pkg.binary_dilation, pkg.binary_erosion, pkg.binary_opening, pkg.binary_closing, pkg.binary_contour,
               pkg.binary_fill_holes):
        with pytest.raises(ValueError, match="connectivity"):
            fn(x, connectivity=4)
        with pytest.raises(ValueError, match="3-D volumes"):
            fn(torch.zeros(4, 4, 4))
        with pytest.raises(NotImplementedError, match="at most 16 channels"):
            fn(torch.zeros(1, 17, 2, 2, 2))
        with pytest.raises(ValueError, match="float32, uint8 or bool"):
            fn(x.double())
    for fn in (pkg.binary_dilation, pkg.binary_erosion):
        with pytest.raises(ValueError, match="border_value"):
            fn(x, border_value=2)
    with pytest.raises(ValueError, match="connectivity"):
        pkg.FillHoles(connectivity=4)
    with pytest.raises(NotImplementedError, match="go up to 31"):
        pkg.FillHoles(applied_labels=[1, 32])
    with pytest.raises(ValueError, match="class-id map"):
        pkg.FillHoles()(torch.zeros(1, 2, 4, 4, 4))
    with pytest.raises(ValueError, match="class-id map"):
        pkg.FillHoles()(torch.zeros(1, 4, 4))


def test_limits_and_no_cpu_fallback(pkg):
    with pytest.raises(NotImplementedError, match="1024 voxels along each axis"):
        pkg.binary_dilation(torch.zeros(1, 1, 1, 1, 1025, dtype=torch.uint8))
    with pytest.raises(NotImplementedError, match="65535 masks"):
        pkg.binary_erosion(torch.zeros(4096, 16, 1, 1, 1, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="ROCm device"):
        pkg.binary_dilation(torch.zeros(1, 1, 4, 4, 4))
    with pytest.raises(RuntimeError, match="ROCm device"):
        pkg.FillHoles()(torch.zeros(1, 1, 4, 4, 4))


def test_exports(pkg):
    for n in NAMES:
        assert n in pkg.__all__ and callable(getattr(pkg, n))
    assert pkg.morphology.MORPH_FUSED >= 1 and pkg.morphology.MORPH_TILE >= 1


# ------------------------------------------------------------------------------------------- the reference's identities
@pytest.mark.parametrize("connectivity", [1, 2, 3])
@pytest.mark.parametrize("border", [0, 1])
def test_erosion_is_the_dual_of_dilation(connectivity, border):
    """the kernel runs erosion as the dilation of the complement under the complemented border"""
    m = rand_mask((2, 2, 6, 7, 9), 0.8, 3)
    for n in (1, 2):
        assert np.array_equal(ref.erosion(m, n, connectivity, border), 1 - ref.dilation(1 - m, n, connectivity, 1 - border))


@pytest.mark.parametrize("connectivity", [1, 2, 3])
def test_fill_holes_is_the_face_restatement(connectivity):
    shell = np.zeros((1, 1, 9, 9, 12), np.uint8)
    shell[0, 0, 2:7, 2:7, 2:10] = 1
    shell[0, 0, 3:6, 3:6, 3:9] = 0
    for m in (rand_mask((2, 2, 8, 9, 10), 0.6, 5), rand_mask((1, 1, 12, 5, 7), 0.75, 6), shell):
        got = ref.fill_holes_restated(m, connectivity)
        assert np.array_equal(got, ref.fill_holes(m, connectivity))
    assert ref.fill_holes(shell, connectivity).sum() - shell.sum() == 3 * 3 * 6


def nest():
    """label 2 around label 1 around a hole, and a second hole inside label 2 that also touches label 1's block"""
    ids = np.zeros((1, 1, 13, 13, 13), np.float32)
    ids[0, 0, 1:12, 1:12, 1:12] = 2
    ids[0, 0, 3:10, 3:10, 3:10] = 1
    ids[0, 0, 6, 6, 6] = 0                  # inside label 1: fills with 1
    ids[0, 0, 2, 5, 5] = 0                  # between label 2 (five neighbours) and label 1 (one): stays
    return ids


def test_fill_holes_rule_on_a_nest():
    ids = nest()
    want = ids.copy()
    want[0, 0, 6, 6, 6] = 1
    for connectivity in (None, 1, 2, 3):
        assert np.array_equal(ref.fill_holes_rule(ids, None, connectivity), want)
    assert np.array_equal(ref.fill_holes_rule(ids, [2], None), ids)
    assert np.array_equal(ref.fill_holes_rule(ids, [1], None), want)


# ------------------------------------------------------------------------------------- the bit-packed step, in numpy
U64 = np.uint64
ALL = U64(0xFFFFFFFFFFFFFFFF)


def pack(m):
    """[D, H, W] bool -> [D, H, nw] uint64, bit b of word w = voxel x = 64 w + b; the bits at x >= W are left as 0"""
    D, H, W = m.shape
    nw = -(-W // 64)
    padded = np.zeros((D, H, nw * 64), bool)
    padded[..., :W] = m
    weights = U64(1) << np.arange(64, dtype=U64)
    return (padded.reshape(D, H, nw, 64).astype(U64) * weights).sum(-1, dtype=U64)


def unpack(p, W):
    bits = (p[..., None] >> np.arange(64, dtype=U64)) & U64(1)
    return bits.reshape(p.shape[0], p.shape[1], -1)[..., :W].astype(bool)


def step(p, W, connectivity, border, erode):
    """one iteration on a packed image, by the word formulas of the issue / DESIGN.md section 22"""
    flip = ALL if erode else U64(0)
    fill = (ALL if border else U64(0)) ^ flip
    tail = (ALL >> U64(64 - W % 64)) if W % 64 else ALL

    def trusted(a):                                   # the bits at x >= W read as the border
        a = a.copy()
        a[..., -1] = (a[..., -1] & tail) | (fill & ~tail)
        return a

    a = np.pad(trusted(p ^ flip), ((1, 1), (1, 1), (0, 0)), constant_values=fill)
    D, H = p.shape[:2]
    row = lambda dz, dy: a[1 + dz:1 + dz + D, 1 + dy:1 + dy + H]
    axis = row(-1, 0) | row(1, 0) | row(0, -1) | row(0, 1)
    diag = row(-1, -1) | row(-1, 1) | row(1, -1) | row(1, 1)
    if connectivity == 1:
        xd, plain = row(0, 0), axis
    elif connectivity == 2:
        xd, plain = row(0, 0) | axis, diag
    else:
        xd, plain = row(0, 0) | axis | diag, np.zeros_like(axis)
    left = np.concatenate([np.full_like(xd[..., :1], fill), xd[..., :-1]], -1)
    right = np.concatenate([xd[..., 1:], np.full_like(xd[..., :1], fill)], -1)
    out = plain | xd | (xd << U64(1)) | (left >> U64(63)) | (xd >> U64(1)) | (right << U64(63))
    return trusted(out) ^ flip


@pytest.mark.parametrize("W", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("connectivity", [1, 2, 3])
@pytest.mark.parametrize("border", [0, 1])
def test_packed_step_model_matches_scipy(pkg, W, connectivity, border):
    assert pkg.morphology.MORPH_FUSED == 4 and pkg.morphology.MORPH_TILE == 8      # what csrc/morphology.hip is built with
    for erode, density in ((0, 0.1), (1, 0.9)):
        m = rand_mask((4, 5, W), density, 10 * W + erode).astype(bool)
        assert np.array_equal(unpack(pack(m), W), m)
        p = pack(m)
        if W % 64:
            p[..., -1] |= ~(ALL >> U64(64 - W % 64)) & U64(0x5A5A5A5A5A5A5A5A)      # padding bits hold anything
        for n in (1, 2, 3):
            p = step(p, W, connectivity, border, erode)
            fn = ndimage.binary_erosion if erode else ndimage.binary_dilation
            want = fn(m, ref.structure(connectivity), n, border_value=border)
            assert np.array_equal(unpack(p, W), want), (erode, n)
