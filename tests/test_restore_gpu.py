"""GPU checks of preprocess.restore_native / VolumeCache.restore (csrc/restore.hip) against the float64 restatement of
tests/restore_ref.py: exact nearest picks wherever the float64 coordinate is not a rounding tie (and no ties in the main
inputs), bit-exact pure reorientations and round trips, trilinear scores within the fp32 blend's rounding, the fused argmax /
sigmoid / BraTS outputs equal to the unfused ones bit for bit, the crop box and its shell, border clamping, every row-offset
residue and brick shape, red zones, and graph capture."""
import dataclasses

import numpy as np
import pytest
import torch

import preprocess_ref as R
import restore_ref as RR
from guard import Guard

pytestmark = pytest.mark.gpu

# native 0.8 x 0.8 x 2.4 mm -> 1 mm: no i * k is a half-integer, so every voxel is compared.  With (0.8, 0.8, 2.5) every odd index
# along the 2.5 mm axis is a rounding tie of the inverse (2.5 i is a half-integer: 44 % of the voxels of this shape); that is the
# deliberate tie case below.
SPACING, TIE_SPACING, ORIGIN, SHAPE = (0.8, 0.8, 2.4), (0.8, 0.8, 2.5), (-12.5, 7.25, 3.0), (11, 13, 9)
# max |gpu - ref| / max |input| of the trilinear scores: fp32 weights from fp64 coordinates and an eight-term fp32 blend, the
# 16 * 2**-24 = 1e-6 that tests/test_preprocess_gpu.py derives for the same arithmetic
LINEAR_REL_BOUND = 1e-6
assert 16 * 2.0 ** -24 <= LINEAR_REL_BOUND


def _bits(t):
    return t.contiguous().view(torch.int32)


def _geom(pkg, native, full, minv, origin=(0, 0, 0), crop=None):
    """a Geometry with an explicit inverse matrix (forward = its inverse): geometries that no affine + pixdim produces"""
    fwd = np.linalg.inv(RR.as4x4(minv))
    return pkg.Geometry(native_shape=tuple(native), affine=np.eye(4), pixdim=(1.0, 1.0, 1.0), axcodes="RAS", full_shape=tuple(full),
                        forward=fwd, oriented_affine=np.eye(4), crop_origin=tuple(origin), crop_shape=tuple(crop or full))


def _ref(x, g, mode):
    return RR.restore(np.asarray(x), g.inverse_matrix(), g.native_shape, g.full_shape, g.crop_origin, mode)


def _geometries(pkg, spacing, angle):
    """the 48 signed permutations, each uncropped and once more with a box one voxel inside the full grid on all six sides"""
    for n, A in enumerate(R.signed_permutation_affines(spacing, ORIGIN, angle)):
        g = pkg.preprocess.geometry(SHAPE, A, (1.0, 1.0, 1.0), "RAS")
        yield n, g
        if n % 4 == 0:
            yield n, g.cropped((1, 1, 1), tuple(f - 2 for f in g.full_shape))


def _scores(rng, C, shape, scale=3.0):
    return torch.as_tensor(rng.standard_normal((C, *shape)) * scale, dtype=torch.float32)


# ---------------------------------------------------------------- 1. nearest
def _nearest_body(pkg, dev, angle):
    rng = np.random.default_rng(100 + int(angle * 100))
    for n, g in _geometries(pkg, SPACING, angle):
        assert RR.ties(g.inverse_matrix(), SHAPE, g.full_shape).mean() == 0          # every voxel is compared
        u8 = torch.as_tensor(rng.integers(1, 256, (3, *g.crop_shape)), dtype=torch.uint8)
        f32 = u8.float() * 1.5 - 100.25
        for C in (1, 3):
            gu = pkg.restore_native(u8[:C].to(dev), g)
            gf = pkg.restore_native(f32[:C].to(dev), g, mode="nearest")
            assert gu.dtype == torch.uint8 and gf.dtype == torch.float32 and tuple(gu.shape) == tuple(gf.shape) == (C, *SHAPE)
            assert np.array_equal(gu.cpu().numpy().astype(np.float64), _ref(u8[:C], g, "nearest")), f"case {n} uint8 C={C}"
            assert np.array_equal(gf.cpu().numpy().astype(np.float64), _ref(f32[:C], g, "nearest")), f"case {n} float32 C={C}"


@pytest.mark.parametrize("angle", [0.0, 0.04])
def test_nearest_exact_over_all_orientations(pkg, dev, angle):
    _nearest_body(pkg, dev, angle)


def test_ties_stay_in_range_and_off_tie_voxels_exact(pkg, dev):
    """(0.8, 0.8, 2.5) mm: 2.5 i is a half-integer for every odd i, which float64 formulations resolve by rounding noise.  Only
    the other voxels are compared; a tie voxel must still pick one of the grid points around its coordinate."""
    rng = np.random.default_rng(7)
    for A in R.signed_permutation_affines(TIE_SPACING, ORIGIN, 0.0)[::5]:
        g = pkg.preprocess.geometry(SHAPE, A)
        Minv = g.inverse_matrix()
        tie = RR.ties(Minv, SHAPE, g.full_shape)
        assert 0.3 < tie.mean() < 0.6, tie.mean()
        lab = torch.as_tensor(rng.integers(0, 200, (1, *g.full_shape)), dtype=torch.uint8)
        got = pkg.restore_native(lab.to(dev), g).cpu().numpy().reshape(-1).astype(np.float64)
        assert np.array_equal(got[~tie], _ref(lab, g, "nearest").reshape(-1)[~tie])
        s = RR.coords(Minv, SHAPE, g.full_shape)
        lo, hi = np.floor(s).astype(int), np.ceil(s).astype(int)
        ln = lab.numpy()[0].astype(np.float64)
        around = np.stack([ln[(hi if a else lo)[:, 0], (hi if b else lo)[:, 1], (hi if c else lo)[:, 2]]
                           for a in (0, 1) for b in (0, 1) for c in (0, 1)])
        assert (around == got[None]).any(0).all()


# ---------------------------------------------------------------- 2. pure reorientation
@pytest.mark.parametrize("shape", [(11, 13, 9), (5, 33, 64)])
def test_pure_reorientation_is_bit_exact(pkg, dev, shape):
    """1 mm data was copied forward, so it is copied back: an all-integer matrix returns the source's bits in every mode"""
    rng = np.random.default_rng(9)
    for n, A in enumerate(R.signed_permutation_affines((1.0, 1.0, 1.0), ORIGIN, 0.0)):
        g = pkg.preprocess.geometry(shape, A)
        Minv = g.inverse_matrix()
        assert np.array_equal(Minv, np.rint(Minv))
        x = _scores(rng, 2, g.full_shape, 200.0)
        x[0, 0, 0, :4] = torch.tensor([-0.0, float("inf"), float("-inf"), float("nan")])
        x[1, -1, -1, -1] = -0.0
        idx = _ref(np.arange(x[0].numel(), dtype=np.float64).reshape(1, *g.full_shape), g, "nearest")[0].astype(np.int64)
        want = _bits(x).reshape(2, -1)[:, torch.as_tensor(idx).reshape(-1)].reshape(2, *shape)
        for mode in ("nearest", "linear"):
            got = pkg.restore_native(x.to(dev), g, mode=mode)
            assert torch.equal(_bits(got.cpu()), want), f"case {n} {mode}"
        # the round trip: what resample_orient made of a native volume comes back as that volume
        v = _scores(rng, 2, shape, 200.0)
        v[1, 0, 0, :4] = torch.tensor([float("nan"), -0.0, float("inf"), float("-inf")])
        fwd, _, _ = pkg.resample_orient(v.to(dev), None, A)
        assert torch.equal(_bits(pkg.restore_native(fwd, g).cpu()), _bits(v)), f"case {n} round trip"


# ---------------------------------------------------------------- 3. linear scores
def _linear_body(pkg, dev, angle):
    rng = np.random.default_rng(300 + int(angle * 100))
    worst = 0.0
    for n, g in _geometries(pkg, SPACING, angle):
        x = _scores(rng, 4, g.crop_shape, 50.0)
        got = pkg.restore_native(x.to(dev), g, mode="linear")
        assert got.dtype == torch.float32 and tuple(got.shape) == (4, *SHAPE)
        worst = max(worst, np.abs(got.cpu().numpy().astype(np.float64) - _ref(x, g, "linear")).max() / float(x.abs().max()))
    return worst


@pytest.mark.parametrize("angle", [0.0, 0.04])
def test_linear_scores_close_to_float64(pkg, dev, angle):
    worst = _linear_body(pkg, dev, angle)
    print(f"angle {angle}: linear max|gpu - ref| / max|input| over the orientations = {worst:.3e}")
    assert worst <= LINEAR_REL_BOUND, worst


# ---------------------------------------------------------------- 4. fused equals unfused
def _fused_body(pkg, dev, C):
    rng = np.random.default_rng(400 + C)
    geoms = [g for n, g in _geometries(pkg, SPACING, 0.04) if n % 7 == 0]
    geoms += [g for n, g in _geometries(pkg, (1.0, 1.0, 1.0), 0.0) if n % 16 == 4]          # the one-tap path
    assert any(g.crop_origin != (0, 0, 0) for g in geoms)
    for g in geoms:
        x = _scores(rng, C, g.crop_shape, 2.0)
        x[:, ::3, ::2] = x[0, ::3, ::2]                                              # exact ties between all channels
        xd = x.to(dev)
        plain = pkg.restore_native(xd, g, mode="linear").cpu()
        inside = torch.as_tensor(RR.inside_mask(g.inverse_matrix(), SHAPE, g.full_shape, g.crop_origin, g.crop_shape).reshape(SHAPE))
        am = pkg.restore_native(xd, g, mode="linear", post="argmax").cpu()
        sg = pkg.restore_native(xd, g, mode="linear", post="sigmoid").cpu()
        assert am.dtype == sg.dtype == torch.uint8 and tuple(am.shape) == (1, *SHAPE) and tuple(sg.shape) == (C, *SHAPE)
        want_am = torch.as_tensor(RR.argmax_first(plain.numpy()))                    # numpy's argmax: the first maximal channel
        assert torch.equal(am, want_am)
        assert torch.equal(sg, ((plain >= 0) & inside[None]).to(torch.uint8))
        if inside.all():
            assert torch.equal(sg, (plain >= 0).to(torch.uint8))
        if C == 4:
            for post in ("argmax", "sigmoid"):
                lab = pkg.restore_native(xd, g, mode="linear", post=post, label_converter="brats").cpu()
                assert lab.dtype == torch.uint8 and tuple(lab.shape) == (1, *SHAPE)
                assert np.array_equal(lab.numpy(), RR.brats_label(RR.discrete(plain.numpy(), inside.numpy(), post))), post
            # nearest one-hot / multi-label channels (float32 and uint8) through the same rule
            oh = (torch.as_tensor(rng.random((4, *g.crop_shape))) < 0.4)
            want = RR.brats_label(_ref(oh.numpy(), g, "nearest") == 1)
            for src in (oh.float(), oh.to(torch.uint8)):
                lab = pkg.restore_native(src.to(dev), g, label_converter="brats").cpu()
                assert lab.dtype == torch.uint8 and np.array_equal(lab.numpy(), want)


@pytest.mark.parametrize("C", [2, 4, 14, 16])
def test_fused_outputs_equal_unfused(pkg, dev, C):
    _fused_body(pkg, dev, C)


# ---------------------------------------------------------------- 5. argmax against float64
def _smooth_scores(C, shape, seed):
    """low-frequency seeded scores: a few plane waves per channel, so class boundaries are surfaces and near-ties are rare"""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    out = np.zeros((C, *shape))
    for c in range(C):
        for _ in range(3):
            k = rng.uniform(-0.35, 0.35, 3)
            out[c] += rng.uniform(0.5, 2.0) * np.sin(k[0] * z + k[1] * y + k[2] * x + rng.uniform(0, 2 * np.pi))
    return out.astype(np.float32)


@pytest.mark.parametrize("C", [2, 14])
def test_argmax_equals_float64_off_near_ties(pkg, dev, C):
    native, excluded, total = (23, 19, 14), 0, 0
    for n, A in enumerate(R.signed_permutation_affines(SPACING, ORIGIN, 0.04)[::6]):
        g = pkg.preprocess.geometry(native, A)
        x = _smooth_scores(C, g.full_shape, 500 + n)
        ref = _ref(x, g, "linear")
        near = RR.top_two_gap(ref) <= 2e-6 * float(np.abs(x).max())                  # twice the blend bound
        got = pkg.restore_native(torch.as_tensor(x).to(dev), g, mode="linear", post="argmax").cpu().numpy()
        assert np.array_equal(got[0][~near], RR.argmax_first(ref)[0][~near]), f"case {n}"
        excluded, total = excluded + int(near.sum()), total + near.size
    print(f"C={C}: {excluded} of {total} voxels excluded as near-ties of the float64 reference ({excluded / total:.2e})")
    assert excluded / total <= 1e-3


# ---------------------------------------------------------------- 6. crop box
def test_crop_box_from_the_cache(pkg, dev):
    """a scan whose foreground box is strictly inside the resampled grid on all six sides, through VolumeCache.add_raw"""
    rng = np.random.default_rng(6)
    shape = (14, 12, 10)
    A = R.signed_permutation_affines((1.2, 1.4, 2.4), ORIGIN, 0.0)[29]              # 1 mm is finer on every axis
    img = torch.zeros(1, *shape)
    lab = torch.zeros(1, *shape, dtype=torch.uint8)
    img[0, 3:10, 3:9, 2:7] = torch.as_tensor(rng.random((7, 6, 5)) + 0.5, dtype=torch.float32)
    lab[0, 3:10, 3:9, 2:7] = torch.as_tensor(rng.integers(0, 5, (7, 6, 5)), dtype=torch.uint8)
    cache = pkg.VolumeCache(dev)
    i = cache.add_raw(img.to(dev), lab.to(dev), A, crop_foreground=True)
    g = cache.geometry(i)
    assert isinstance(g, pkg.Geometry) and g.native_shape == shape and g.crop_shape == tuple(cache.shapes[i][2:])
    assert all(o > 0 and o + c < f for o, c, f in zip(g.crop_origin, g.crop_shape, g.full_shape)), "strictly inside on six sides"
    assert np.array_equal(g.oriented_affine, cache.affine(i)) and np.array_equal(g.affine, A)
    Minv = g.inverse_matrix()
    inside = RR.inside_mask(Minv, shape, g.full_shape, g.crop_origin, g.crop_shape).reshape(shape)
    s = RR.coords(Minv, shape, g.full_shape)
    f = np.floor(s)
    o, c = np.array(g.crop_origin), np.array(g.crop_shape)
    interior = ((f >= o) & (f + 1 <= o + c - 1)).all(1).reshape(shape)
    shell = inside & ~interior
    assert (~inside).any() and shell.any() and interior.any()
    assert RR.ties(Minv, shape, g.full_shape).mean() == 0

    x = _scores(rng, 4, g.crop_shape, 2.0) + 1.0
    xd = x.to(dev)
    outs = {"nearest": cache.restore(i, xd), "linear": cache.restore(i, xd, mode="linear"),
            "argmax": cache.restore(i, xd, mode="linear", post="argmax"), "sigmoid": cache.restore(i, xd, mode="linear", post="sigmoid"),
            "argmax+brats": cache.restore(i, xd, mode="linear", post="argmax", label_converter="brats"),
            "sigmoid+brats": cache.restore(i, xd, mode="linear", post="sigmoid", label_converter="brats"),
            "u8": cache.restore(i, (x > 1).to(torch.uint8).to(dev)), "5d": cache.restore(i, xd[None], mode="linear")}
    for name, t in outs.items():
        assert not t.cpu()[:, torch.as_tensor(~inside)].any(), f"{name}: a voxel outside the box is not 0"
    lin = outs["linear"].cpu().numpy().astype(np.float64)
    ref = _ref(x, g, "linear")
    assert np.abs(lin - ref).max() / float(x.abs().max()) <= LINEAR_REL_BOUND
    assert np.abs(lin - ref)[:, shell].max() / float(x.abs().max()) <= LINEAR_REL_BOUND      # taps clamped into the box
    assert torch.equal(outs["5d"], outs["linear"])
    assert np.array_equal(outs["nearest"].cpu().numpy().astype(np.float64), _ref(x, g, "nearest"))
    assert np.array_equal(outs["sigmoid"].cpu().numpy(), ((lin >= 0) & inside[None]).astype(np.uint8))
    # the label the cache holds, taken back: the scan's own label (the grid is finer, so every native voxel finds itself again)
    back = cache.restore(i, cache.label(i))
    assert back.dtype == torch.uint8 and torch.equal(back.cpu(), lab)
    with pytest.raises(ValueError, match="no affine"):
        direct = pkg.VolumeCache(dev)
        direct.add(img.to(dev), lab.to(dev))
        direct.geometry(0)
    with pytest.raises(IndexError):
        cache.geometry(3)


# ---------------------------------------------------------------- 7. border clamp
@pytest.mark.parametrize("native", [(17, 15, 24), (16, 14, 23)])
def test_border_clamping_at_all_six_faces(pkg, dev, native):
    """test_preprocess_gpu's overhanging geometry, backwards: the native grid overhangs the resampled one on every face"""
    full = (9, 8, 11)
    minv = np.array([[0.0, 0.0, 0.77, -3.4], [0.0, -0.95, 0.0, 9.7], [0.93, 0.0, 0.0, -2.6]])
    g = _geom(pkg, native, full, minv)
    Minv = g.inverse_matrix()
    assert np.abs(Minv - minv).max() < 1e-12
    s = np.stack(np.meshgrid(*[np.arange(n) for n in native], indexing="ij"), -1).reshape(-1, 3) @ Minv[:, :3].T + Minv[:, 3]
    for a in range(3):
        assert s[:, a].min() < -1 and s[:, a].max() > full[a]
    assert RR.ties(Minv, native, full).mean() == 0
    rng = np.random.default_rng(21)
    x = _scores(rng, 2, full, 100.0)
    lab = torch.as_tensor(rng.integers(0, 200, (1, *full)), dtype=torch.uint8)
    gi = pkg.restore_native(x.to(dev), g, mode="linear").cpu()
    gl = pkg.restore_native(lab.to(dev), g).cpu()
    assert np.array_equal(gl.numpy().astype(np.float64), _ref(lab, g, "nearest"))
    assert np.abs(gi.numpy() - _ref(x, g, "linear")).max() / float(x.abs().max()) <= LINEAR_REL_BOUND
    # the corner voxels of the native grid are the resampled grid's corner voxels themselves
    assert gi[0, 0, 0, 0] == x[0, 0, -1, 0] and gi[1, -1, -1, -1] == x[1, -1, 0, -1]


# ---------------------------------------------------------------- 8. row shapes and brick choices
_ROW_SHAPES = [(5, 7, 1), (5, 3, 3), (3, 5, 4), (3, 3, 5), (2, 3, 7), (17, 9, 70), (2, 1, 70)]


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_row_offsets_brick_edges_and_brick_choice(pkg, dev, axis):
    """native rows of 1, 3, 4, 5, 7 and 70 voxels (row offsets of every residue mod 4), volumes below one brick and across brick
    edges on every axis, and each of the three brick shapes: `axis` is the native axis the source's fastest axis moves along"""
    rng = np.random.default_rng(80 + axis)
    residues = set()
    for native in _ROW_SHAPES:
        perm = {0: (2, 1, 0), 1: (0, 2, 1), 2: (0, 1, 2)}[axis]                      # source axis a follows native axis perm[a]
        scale = (0.83, 1.21, 0.91)
        full = tuple(max(2, int(round(native[perm[a]] * scale[a]))) for a in range(3))
        minv = np.zeros((3, 4))
        for a in range(3):
            minv[a, perm[a]], minv[a, 3] = scale[a], 0.125 + 0.25 * a      # no i * scale + offset is a half-integer
        g = _geom(pkg, native, full, minv, (0, 1, 0), (full[0], full[1] - 1, full[2])) if full[1] > 2 else _geom(pkg, native, full, minv)
        Minv = g.inverse_matrix()
        assert int(np.argmax(np.abs(Minv[2, :3]))) == axis                           # the brick the entry point chooses
        assert RR.ties(Minv, native, full).mean() == 0
        residues |= {((z * native[1] + y) * native[2]) % 4 for z in range(native[0]) for y in range(native[1])}
        x = _scores(rng, 2, g.crop_shape, 10.0)
        xd = x.to(dev)
        lin = pkg.restore_native(xd, g, mode="linear")
        near = pkg.restore_native(xd, g)
        am = pkg.restore_native(xd, g, mode="linear", post="argmax")
        ref = _ref(x, g, "linear")
        assert np.abs(lin.cpu().numpy() - ref).max() / float(x.abs().max()) <= LINEAR_REL_BOUND, native
        assert np.array_equal(near.cpu().numpy().astype(np.float64), _ref(x, g, "nearest")), native
        assert torch.equal(am.cpu(), torch.as_tensor(RR.argmax_first(lin.cpu().numpy()))), native
        # out= at an offset that is not a multiple of 4 bytes (bytes) / 16 bytes (floats): element-wise stores, the same values
        nf, nb = lin.numel(), am.numel()
        fbuf = torch.full((nf + 9,), float("nan"), device=dev)
        bbuf = torch.full((nb + 9,), 0x5A, dtype=torch.uint8, device=dev)
        fo, bo = fbuf[1:1 + nf].view(lin.shape), bbuf[1:1 + nb].view(am.shape)
        assert fo.data_ptr() % 16 == 4 and bo.data_ptr() % 4 == 1
        assert pkg.restore_native(xd, g, mode="linear", out=fo) is fo
        assert pkg.restore_native(xd, g, mode="linear", post="argmax", out=bo) is bo
        assert torch.equal(_bits(fo), _bits(lin)) and torch.equal(bo, am)
        assert fbuf[0].isnan() and fbuf[1 + nf:].isnan().all() and (bbuf[0] == 0x5A) and (bbuf[1 + nb:] == 0x5A).all()
    assert residues == {0, 1, 2, 3}


def test_c_entry_point_refuses_bad_arguments(pkg, dev):
    lib = pkg._capi.load()
    G = pkg._capi.RestoreGeom
    x = torch.zeros(4, 8, 8, 8, device=dev)
    out = torch.zeros(4, 8, 8, 8, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def geom(full=(8, 8, 8), origin=(0, 0, 0), crop=(8, 8, 8), m=(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)):
        g = G()
        g.m[:], g.full[:], g.origin[:], g.crop[:] = [float(v) for v in m], full, origin, crop
        return g

    def rc(src=x.data_ptr(), u8=0, C=4, g=None, n=(8, 8, 8), linear=0, post=0, brats=0, o=out.data_ptr()):
        return lib.unetr_restore_native(src, u8, C, g or geom(), *n, linear, post, brats, o, st)
    assert rc() == 0 and rc(linear=1) == 0 and rc(linear=1, post=1) == 0 and rc(linear=1, post=2, brats=1) == 0 and rc(brats=1) == 0
    assert rc(src=None) == 1 and rc(o=None) == 1 and rc(C=0) == 1 and rc(C=17) == 1 and rc(n=(0, 8, 8)) == 1
    assert rc(post=1) == 1 and rc(linear=1, post=3) == 1 and rc(u8=1, linear=1) == 1
    assert rc(C=3, brats=1) == 1 and rc(linear=1, brats=1) == 1
    assert rc(g=geom(origin=(1, 0, 0))) == 1 and rc(g=geom(crop=(0, 8, 8))) == 1 and rc(g=geom(m=(float("nan"),) + (0,) * 11)) == 1
    # 2**31 voxels on either grid and a launch-grid dimension over 65535 are refused before anything is launched
    assert rc(n=(2048, 2048, 512)) == 3 and rc(g=geom(full=(2048, 2048, 512))) == 3
    assert rc(n=(8, 65536 * 8, 8)) == 3
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 9. red zones
def test_inside_red_zones(pkg, dev):
    """items 1, 3 and 4 again with every device tensor between poisoned red zones and every fresh output poisoned: no red
    zone may change, and a voxel the kernel did not write (background included) would reach the comparisons as poison"""
    with Guard(dev) as gd:
        _nearest_body(pkg, dev, 0.04)
        worst = _linear_body(pkg, dev, 0.04)
        _fused_body(pkg, dev, 4)
        _fused_body(pkg, dev, 14)
    assert worst <= LINEAR_REL_BOUND
    assert gd.check() > 0


# ---------------------------------------------------------------- 10. stream order
def test_graph_capture_equals_eager(pkg, dev):
    rng = np.random.default_rng(10)
    A = R.signed_permutation_affines(SPACING, ORIGIN, 0.04)[13]
    g = pkg.preprocess.geometry(SHAPE, A)
    g = g.cropped((1, 0, 2), tuple(f - 2 for f in g.full_shape))
    src = _scores(rng, 4, g.crop_shape).to(dev)
    out = torch.full((1, *SHAPE), 0x5A, dtype=torch.uint8, device=dev)
    kw = dict(mode="linear", post="argmax", label_converter="brats")
    torch.cuda.set_sync_debug_mode("error")
    try:
        pkg.restore_native(src, g, out=out, **kw)                                   # no synchronising call inside
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pkg.restore_native(src, g, out=out, **kw)
    for _ in range(3):
        new = _scores(rng, 4, g.crop_shape).to(dev)
        src.copy_(new)
        out.fill_(0x5A)
        graph.replay()
        assert torch.equal(out, pkg.restore_native(new, g, **kw))
    assert dataclasses.is_dataclass(g)
