"""GPU checks of preprocess.resample_orient / VolumeCache.add_raw (csrc/preprocess.hip) against the float64 restatement of
tests/preprocess_ref.py: exact labels wherever the float64 source coordinate is not a rounding tie (and no ties in the main
inputs), the image within the fp32 blend's rounding, bit-exact int16 / multi-channel / pure-reorientation paths, border
clamping, the BraTS converter, the cache built from raw volumes, and the error paths."""
import ctypes

import numpy as np
import pytest
import torch

import augment_ref as AR
import preprocess_ref as R

pytestmark = pytest.mark.gpu

SPACING, ORIGIN, SHAPE = (0.79, 0.83, 2.3), (-12.5, 7.25, 3.0), (20, 18, 9)
# max |gpu - ref| / max |input| of the trilinear image.  Measured on the MI355X over the 96 cases of
# test_all_orientations_labels_exact_image_close: 1.313e-7; the bound is 4x that.  fp32 weights and an
# 8-term fp32 blend allow about 16 * 2**-24 = 1e-6, and anything above 1e-5 would be a bug, not a tolerance.
IMAGE_REL_BOUND = 4 * 1.313e-7
assert IMAGE_REL_BOUND < 1e-5


def _volume(shape, seed, C=1):
    rng = np.random.default_rng(seed)
    return (torch.as_tensor(rng.random((C, *shape)) * 400 - 200, dtype=torch.float32),
            torch.as_tensor(rng.integers(0, 4, (1, *shape)), dtype=torch.uint8))


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("angle", [0.0, 0.04])
def test_all_orientations_labels_exact_image_close(pkg, dev, angle):
    worst = 0.0
    for n, A in enumerate(R.signed_permutation_affines(SPACING, ORIGIN, angle)):
        x, lab = _volume(SHAPE, n)
        y, aff, TM = R.library_route(x, A, (1, 1, 1), "RAS", "bilinear")
        yl, _, _ = R.library_route(lab, A, (1, 1, 1), "RAS", "nearest")
        tie = R.tie_mask(TM, y.shape[1:], SHAPE).mean()
        assert tie == 0, tie                          # every label voxel is compared
        gi, gl, gaff = pkg.resample_orient(x.to(dev), lab.to(dev), A, (1.0, 1.0, 1.0), "RAS")
        assert gi.dtype == torch.float32 and gl.dtype == torch.uint8 and tuple(gi.shape) == y.shape and tuple(gl.shape) == yl.shape
        assert np.array_equal(gl.cpu().numpy().astype(np.float64), yl), f"case {n}"
        assert np.abs(gaff - aff).max() <= 1e-12
        err = np.abs(gi.cpu().numpy().astype(np.float64) - y).max() / float(x.abs().max())
        worst = max(worst, err)
    print(f"angle {angle}: image max|gpu - ref| / max|input| over 48 orientations = {worst:.3e}")
    assert worst <= IMAGE_REL_BOUND, worst


def test_ties_stay_in_range_and_off_tie_voxels_exact(pkg, dev):
    """spacing (0.8, 0.8, 2.5): a large share of the source coordinates are half-integers, which the library's own arithmetic
    resolves by rounding noise.  Only the other voxels are compared; a tie voxel must still pick one of the voxels around it."""
    shape, A = (40, 40, 16), np.diag([0.8, 0.8, 2.5, 1.0])
    A[:3, 3] = ORIGIN
    x, lab = _volume(shape, 7)
    lab = torch.as_tensor(np.random.default_rng(7).integers(0, 200, (1, *shape)), dtype=torch.uint8)
    yl, _, TM = R.library_route(lab, A, (1, 1, 1), "RAS", "nearest")
    out_shape, mat, _ = pkg.preprocess.plan(shape, A)
    tie = R.tie_mask(TM, yl.shape[1:], shape)
    assert np.array_equal(tie, R.tie_mask(np.vstack([mat, [0, 0, 0, 1]]), out_shape, shape))
    assert 0.3 < tie.mean() < 0.6, tie.mean()      # source = 1.25 j on two axes: a half-integer for 1 j in 4, so 1 - (3/4)**2 = 44 % before clamping
    _, gl, _ = pkg.resample_orient(x.to(dev), lab.to(dev), A)
    g = gl.cpu().numpy().reshape(-1).astype(np.float64)
    assert np.array_equal(g[~tie], yl.reshape(-1)[~tie])
    s = R.source_coords(TM, out_shape, shape)
    lo, hi = np.floor(s).astype(int), np.ceil(s).astype(int)
    ln = lab.numpy()[0].astype(np.float64)
    around = np.stack([ln[(hi if a else lo)[:, 0], (hi if b else lo)[:, 1], (hi if c else lo)[:, 2]]
                       for a in (0, 1) for b in (0, 1) for c in (0, 1)])
    assert (around == g[None]).any(0).all()


def test_int16_source_equals_float32_source(pkg, dev):
    rng = np.random.default_rng(11)
    xi = torch.as_tensor(rng.integers(-1024, 3000, (2, 23, 17, 12)), dtype=torch.int16)
    for A in R.signed_permutation_affines(SPACING, ORIGIN, 0.04)[::7]:
        a, _, _ = pkg.resample_orient(xi.to(dev), None, A)
        b, _, _ = pkg.resample_orient(xi.float().to(dev), None, A)
        assert torch.equal(_bits(a), _bits(b))
    A = R.signed_permutation_affines((1.0, 1.0, 1.0), ORIGIN, 0.0)[29]          # the one-tap path
    a, _, _ = pkg.resample_orient(xi.to(dev), None, A)
    b, _, _ = pkg.resample_orient(xi.float().to(dev), None, A)
    assert torch.equal(_bits(a), _bits(b))


def test_four_channels_equal_four_calls(pkg, dev):
    x, lab = _volume((19, 21, 10), 5, C=4)
    for A in R.signed_permutation_affines(SPACING, ORIGIN, 0.04)[3::11]:
        gi, gl, _ = pkg.resample_orient(x.to(dev), lab.to(dev), A)
        for c in range(4):
            gc, glc, _ = pkg.resample_orient(x[c:c + 1].to(dev), lab.to(dev), A)
            assert torch.equal(_bits(gi[c:c + 1]), _bits(gc)) and torch.equal(gl, glc)


@pytest.mark.parametrize("shape", [(20, 18, 9), (16, 12, 8), (5, 33, 64)])
def test_identity_spacing_is_a_bit_exact_flip_transpose(pkg, dev, shape):
    """1 mm data: Spacing copies, the kernel runs on integer coordinates and must hand back the input's bits (-0.0, inf, nan)"""
    x, lab = _volume(shape, 9, C=2)
    x[0, 0, 0, :4] = torch.tensor([-0.0, float("inf"), float("-inf"), float("nan")])
    x[1, -1, -1, -1] = -0.0
    for A in R.signed_permutation_affines((1.0, 1.0, 1.0), ORIGIN, 0.0):
        gi, gl, gaff = pkg.resample_orient(x.to(dev), lab.to(dev), A)
        y, aff, M = R.orientation(x.numpy(), A, "RAS")
        yl, _, _ = R.orientation(lab.numpy(), A, "RAS")
        assert torch.equal(_bits(gi.cpu()), _bits(torch.as_tensor(y)))
        assert torch.equal(gl.cpu(), torch.as_tensor(yl))
        assert np.abs(gaff - aff).max() <= 1e-12 and np.array_equal(R.io_orientation(gaff), [[0, 1], [1, 1], [2, 1]])


def _raw_call(pkg, dev, x, lab, mat, out_shape, L=1, brats=0, oi=None, ol=None):
    """unetr_resample_orient with an explicit matrix, into oi / ol where given"""
    xd = x.to(dev).contiguous()
    ld = lab.to(dev).contiguous()
    oi = torch.full((x.shape[0], *out_shape), float("nan"), device=dev) if oi is None else oi
    ol = torch.full((L, *out_shape), 255, dtype=torch.uint8, device=dev) if ol is None else ol
    m = (ctypes.c_double * 12)(*np.asarray(mat, dtype=np.float64).reshape(-1).tolist())
    pkg._capi.call("unetr_resample_orient", xd.data_ptr(), int(xd.dtype == torch.int16), ld.data_ptr(), x.shape[0], L, brats,
                   *x.shape[1:], m, *out_shape, oi.data_ptr(), ol.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return oi.cpu(), ol.cpu()


@pytest.mark.parametrize("out_shape", [(17, 15, 24), (16, 14, 23)])
def test_border_clamping_at_all_six_faces(pkg, dev, out_shape):
    """an output grid that overhangs the source by several voxels on every face (W % 4 == 0 and the scalar-store tail)"""
    shape = (9, 8, 11)
    x, lab = _volume(shape, 21, C=2)
    mat = np.array([[0.0, 0.0, 0.77, -3.4], [0.0, -0.95, 0.0, 9.7], [0.93, 0.0, 0.0, -2.6]])     # d0 <- x, d1 <- -y, d2 <- z
    M4 = np.vstack([mat, [0, 0, 0, 1]])
    s = np.stack(np.meshgrid(*[np.arange(n) for n in out_shape], indexing="ij"), -1).reshape(-1, 3) @ mat[:, :3].T + mat[:, 3]
    for a in range(3):
        assert s[:, a].min() < -1 and s[:, a].max() > shape[a]
    assert R.tie_mask(M4, out_shape, shape).mean() == 0
    gi, gl = _raw_call(pkg, dev, x, lab, mat, out_shape)
    ref = R.fused_gather(x.numpy(), M4, out_shape, "bilinear")
    assert np.array_equal(gl.numpy().astype(np.float64), R.fused_gather(lab.numpy(), M4, out_shape, "nearest"))
    assert np.abs(gi.numpy() - ref).max() / float(x.abs().max()) <= IMAGE_REL_BOUND
    # the corner output voxels are the source's corner voxels themselves
    assert gi[0, 0, 0, 0] == x[0, 0, -1, 0] and gi[1, -1, -1, -1] == x[1, -1, 0, -1]


_ROW_SHAPES = [(5, 7, 1), (5, 3, 3), (3, 5, 4), (3, 3, 5), (2, 3, 7), (17, 9, 70), (2, 1, 70)]       # as test_restore_gpu's


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_row_ends_unaligned_outputs_and_brick_choice(pkg, dev, axis):
    """output rows of 1, 3, 4, 5, 7 and 70 voxels (row offsets of every residue mod 4), volumes below one brick and across brick
    edges, each of the three brick shapes (`axis` is the output axis the source's fastest axis moves along), two image and two label
    channels so that channel planes start off the 4-voxel boundary, and outputs that start one element past the vector alignment:
    element-wise stores must write the same values and nothing else"""
    rng = np.random.default_rng(60 + axis)
    residues, rows = set(), set()
    for n, out_shape in enumerate(_ROW_SHAPES):
        perm = {0: (2, 1, 0), 1: (0, 2, 1), 2: (0, 1, 2)}[axis]                      # source axis a follows output axis perm[a]
        scale = (0.83, 1.21, 0.91)
        shape = tuple(max(2, int(round(out_shape[perm[a]] * scale[a]))) for a in range(3))
        mat = np.zeros((3, 4))
        for a in range(3):
            mat[a, perm[a]], mat[a, 3] = scale[a], 0.125 + 0.25 * a      # no j * scale + offset is a half-integer
        M4 = np.vstack([mat, [0, 0, 0, 1]])
        assert int(np.argmax(np.abs(mat[2, :3]))) == axis                            # the brick the entry point chooses
        assert R.tie_mask(M4, out_shape, shape).mean() == 0
        residues |= {((z * out_shape[1] + y) * out_shape[2]) % 4 for z in range(out_shape[0]) for y in range(out_shape[1])}
        rows.add(out_shape[2])
        lab = torch.as_tensor(rng.integers(0, 200, (2, *shape)), dtype=torch.uint8)
        sources = [torch.as_tensor(rng.random((2, *shape)) * 400 - 200, dtype=torch.float32)]
        if n == 5:                                                                    # the int16 source once per axis, on several bricks
            sources.append(torch.as_tensor(rng.integers(-1024, 3000, (2, *shape)), dtype=torch.int16))
        want_l = R.fused_gather(lab.numpy(), M4, out_shape, "nearest")
        for x in sources:
            gi, gl = _raw_call(pkg, dev, x, lab, mat, out_shape, L=2)
            err = np.abs(gi.numpy() - R.fused_gather(x.numpy(), M4, out_shape, "bilinear")).max() / float(x.float().abs().max())
            print(f"axis {axis} out {out_shape} {x.dtype}: image max|gpu - ref| / max|input| = {err:.3e}")
            assert np.array_equal(gl.numpy().astype(np.float64), want_l), out_shape
            assert err <= IMAGE_REL_BOUND, (out_shape, err)
            nf, nb = gi.numel(), gl.numel()
            fbuf = torch.full((nf + 9,), float("nan"), device=dev)
            bbuf = torch.full((nb + 9,), 0x5A, dtype=torch.uint8, device=dev)
            fo, bo = fbuf[1:1 + nf].view(gi.shape), bbuf[1:1 + nb].view(gl.shape)
            assert fo.data_ptr() % 16 == 4 and bo.data_ptr() % 4 == 1
            ui, ul = _raw_call(pkg, dev, x, lab, mat, out_shape, L=2, oi=fo, ol=bo)
            assert torch.equal(_bits(ui), _bits(gi)) and torch.equal(ul, gl), out_shape
            assert fbuf[0].isnan() and fbuf[1 + nf:].isnan().all() and (bbuf[0] == 0x5A) and (bbuf[1 + nb:] == 0x5A).all()
    assert residues == {0, 1, 2, 3} and rows == {1, 3, 4, 5, 7, 70}


def test_brats_converter_exact(pkg, dev):
    shape = (22, 24, 15)
    x, lab = _volume(shape, 31, C=4)
    lab[0, :3] = 4                                     # a value outside the BraTS classes: background 0, no class
    for A in R.signed_permutation_affines(SPACING, ORIGIN, 0.04)[5::9] + R.signed_permutation_affines((1, 1, 1), ORIGIN, 0.0)[7::13]:
        want, _, TM = R.library_route(R.brats_channels(lab.numpy()[0]), A, (1, 1, 1), "RAS", "nearest")
        assert R.tie_mask(TM, want.shape[1:], shape).mean() == 0
        _, gl, _ = pkg.resample_orient(x.to(dev), lab.to(dev), A, label_converter="brats")
        assert gl.dtype == torch.uint8 and tuple(gl.shape) == want.shape
        assert np.array_equal(gl.cpu().numpy().astype(np.float64), want)


def _cache_volumes(cache):
    return [(tuple(s[2:]), cache.fg_indices(i).cpu().numpy(), cache.bg_indices(i).cpu().numpy()) for i, s in
            enumerate(cache.shapes)]


def test_add_raw_equals_add_of_resample_orient_and_feeds_the_augment(pkg, dev):
    affs = R.signed_permutation_affines(SPACING, ORIGIN, 0.04)
    raw, direct = pkg.VolumeCache(dev), pkg.VolumeCache(dev)
    for n, (A, shape) in enumerate([(affs[17], (40, 36, 14)), (affs[30], (36, 44, 15))]):
        x, lab = _volume(shape, 40 + n)
        x = x * 5
        kw = dict(scale_range=(-175, 250, 0.0, 1.0), crop_foreground=True)
        i = raw.add_raw(x.to(dev), lab.to(dev), A, pixdim=(1.0, 1.0, 1.0), axcodes="RAS", **kw)
        gi, gl, gaff = pkg.resample_orient(x.to(dev), lab.to(dev), A, (1.0, 1.0, 1.0), "RAS")
        j = direct.add(gi, gl, **kw)
        assert i == j == n and raw.shapes[i] == direct.shapes[j]
        assert torch.equal(raw.image(i), direct.image(j)) and torch.equal(raw.label(i), direct.label(j))
        assert torch.equal(raw.fg_indices(i), direct.fg_indices(j)) and torch.equal(raw.bg_indices(i), direct.bg_indices(j))
        assert np.array_equal(raw.affine(i), gaff) and np.array_equal(R.io_orientation(raw.affine(i)), [[0, 1], [1, 1], [2, 1]])
        with pytest.raises(ValueError, match="no affine"):
            direct.affine(j)
    aug = pkg.RandCropAugment(raw, spatial_size=16, num_samples=4, batch_size=8, pos=1, neg=1, seed=5)
    x = torch.full((8, 1, 16, 16, 16), float("nan"), device=dev)
    y = torch.full((8, 1, 16, 16, 16), float("nan"), device=dev)
    tables = []
    for _ in range(3):
        aug(x, y)
        tables.append(aug.params.cpu().clone())
    ref = AR.replay(AR.aug_config(aug), _cache_volumes(raw), [0, 1], ncalls=3)
    assert all(torch.equal(t, r) for t, r in zip(tables, ref))
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(y).all())


def test_add_raw_brats(pkg, dev):
    shape = (24, 24, 20)
    x, lab = _volume(shape, 50, C=4)
    A = R.signed_permutation_affines((1.0, 1.0, 1.0), ORIGIN, 0.0)[24]            # LPS-like 1 mm grid: pure reorientation
    cache = pkg.VolumeCache(dev)
    i = cache.add_raw(x.to(dev), lab.to(dev), A, label_converter="brats")
    y, _, _ = R.orientation(x.numpy(), A)
    yl, _, _ = R.orientation(lab.numpy(), A)
    assert cache.shapes[i][:2] == (4, 4)
    assert torch.equal(cache.image(i)[0].cpu(), torch.as_tensor(y))
    assert np.array_equal(cache.label(i)[0].cpu().numpy().astype(np.float32), R.brats_channels(yl[0]))


def test_error_paths(pkg, dev):
    x, lab = _volume((8, 8, 8), 1)
    xd, ld = x.to(dev), lab.to(dev)
    A = np.diag([0.8, 0.8, 2.5, 1.0])
    cache = pkg.VolumeCache(dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.resample_orient(x, None, A)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.resample_orient(xd, lab, A)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cache.add_raw(x, lab, A)
    with pytest.raises(ValueError, match="4x4"):
        pkg.resample_orient(xd, ld, np.eye(3))
    with pytest.raises(ValueError, match="pixdim"):
        pkg.resample_orient(xd, ld, A, pixdim=(1.0, -1.0, 1.0))
    with pytest.raises(ValueError, match="pixdim"):
        cache.add_raw(xd, ld, A, pixdim=(0.0, 1.0, 1.0))
    S = A.copy()
    S[:3, 2] = 0.0
    with pytest.raises(ValueError, match="singular"):
        pkg.resample_orient(xd, ld, S)
    with pytest.raises(ValueError, match="one-channel"):
        pkg.resample_orient(xd, ld.expand(2, -1, -1, -1), A, label_converter="brats")
    with pytest.raises(ValueError, match="integers in 0..255"):
        pkg.resample_orient(xd, ld.float() + 0.5, A)
    with pytest.raises(ValueError, match="device and grid"):
        pkg.resample_orient(xd, ld[:, :4], A)
    assert len(cache) == 0
    # the C entry point itself: null pointers, channel counts out of range
    lib = pkg._capi.load()
    m = (ctypes.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    out = torch.empty(1, 8, 8, 8, device=dev)
    ol = torch.empty(4, 8, 8, 8, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def rc(img=xd.data_ptr(), lbl=ld.data_ptr(), C=1, L=1, brats=0, mat=m, oimg=out.data_ptr(), olbl=ol.data_ptr(), n0=8):
        return lib.unetr_resample_orient(img, 0, lbl, C, L, brats, n0, 8, 8, mat, 8, 8, 8, oimg, olbl, st)
    assert rc() == 0
    assert rc(img=None) == 1 and rc(oimg=None) == 1 and rc(mat=None) == 1 and rc(olbl=None) == 1
    assert rc(C=0) == 1 and rc(C=9) == 1 and rc(L=0) == 1 and rc(L=9) == 1 and rc(L=3, brats=1) == 1 and rc(n0=0) == 1
    assert rc(lbl=None, olbl=None, L=0) == 0
    # 2**31 output voxels are refused before anything is launched
    assert lib.unetr_resample_orient(xd.data_ptr(), 0, None, 1, 0, 0, 8, 8, 8, m, 2048, 2048, 512, out.data_ptr(), None, st) == 3
    torch.cuda.synchronize()
