"""CPU anchors of tests/augment_affine_ref.py, the restatement the GPU tests pin csrc/augment.hip's affine gather to: the sign
conventions against torch.rot90 / torch.flip, the float32 interpolation against a float64 evaluation, the matrix against an
independent numpy build, and the replay of the draws."""
import math

import numpy as np
import torch

import augment_affine_ref as A
import augment_ref as R


def _volume(C, L, shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(C, *shape, generator=g), torch.randint(0, 14, (L, *shape), generator=g).to(torch.uint8)


def _quarter_turn(axis, sign=1.0):
    """R_axis(sign * pi / 2) as exact integers: the cyclic analogue of R2 = [[c, -s, 0], [s, c, 0], [0, 0, 1]]"""
    a, b = (axis + 1) % 3, (axis + 2) % 3
    m = np.zeros((3, 3))
    m[axis, axis] = 1.0
    m[a, b], m[b, a] = -sign, sign
    return m


def test_signed_permutations_equal_rot90_and_flip():
    """M an exact signed permutation, a cube crop strictly inside the volume: image and label are torch.rot90 / torch.flip of the
    plain crop, exactly.  out[p] = crop[c + M (p - c)]; for R_axis(+90 deg) over the plane (a, b) = (axis + 1, axis + 2) that is
    out[pa, pb] = crop[n - 1 - pb, pa] = torch.rot90(crop, 1, (b, a)): the sign convention of R0, R1, R2."""
    S, corner = (8, 8, 8), (5, 4, 6)
    img, lbl = _volume(2, 1, (19, 17, 21), seed=1)
    sl = (slice(None),) + tuple(slice(c, c + s) for c, s in zip(corner, S))
    ci, cl = img[sl], lbl[sl].float()
    for axis in range(3):
        a, b = (axis + 1) % 3, (axis + 2) % 3
        for sign, dims in ((1.0, (b + 1, a + 1)), (-1.0, (a + 1, b + 1))):
            x, y = A.affine_sample(img, lbl, corner, S, 0, 0, (0, 1), _quarter_turn(axis, sign))
            assert torch.equal(x, torch.rot90(ci, 1, dims)) and torch.equal(y, torch.rot90(cl, 1, dims)), (axis, sign)
        # the built matrix is the same turn up to the rounding of cos(pi / 2)
        built = A.build_matrix([math.pi / 2 if i == axis else 0.0 for i in range(3)], (1.0, 1.0, 1.0)).reshape(3, 3)
        assert np.abs(built - _quarter_turn(axis)).max() < 1e-7
    for axis in range(3):                                       # a reflection is a flip
        m = np.eye(3)
        m[axis, axis] = -1.0
        x, y = A.affine_sample(img, lbl, corner, S, 0, 0, (0, 1), m)
        assert torch.equal(x, torch.flip(ci, (axis + 1,))) and torch.equal(y, torch.flip(cl, (axis + 1,)))
    # the identity under every flip mask and k is augment_ref's integer path
    for flips in range(8):
        for k in range(4):
            x, y = A.affine_sample(img, lbl, corner, S, flips, k, (0, 1), np.eye(3))
            assert torch.equal(x, R.augment_seq(img, corner, S, flips, k)) and torch.equal(y, R.augment_seq(lbl, corner, S, flips, k).float())


def _trilinear_f64(img, sc):
    """float64 trilinear evaluation at the float32 coordinates sc (border padding), independent of trilinear_f32's order"""
    sc = sc.double()
    out = torch.zeros(img.shape[0], *sc.shape[1:], dtype=torch.float64)
    f = [torch.floor(sc[a]) for a in range(3)]
    for corner in range(8):
        w = torch.ones(sc.shape[1:], dtype=torch.float64)
        idx = []
        for a in range(3):
            bit = corner >> a & 1
            t = sc[a] - f[a]
            w = w * (t if bit else 1.0 - t)
            idx.append((f[a].long() + bit).clamp(0, img.shape[1 + a] - 1))
        out += w * img.double()[:, idx[0], idx[1], idx[2]]
    return out


def test_float32_interpolation_is_within_65_ulp_of_float64():
    """Each lerp a + t * (b - a) in float32, with |a|, |b| <= m and 0 <= t <= 1, makes three roundings: of b - a (|.| <= 2m,
    error <= 2 u m), of the product (carries that error, adds <= 2 u m) and of the sum (<= u m, its result is within m up to
    second order), at most 5 u m with u = 2**-24; an error e on both inputs comes out as at most 3 e ((1 - t) e + t e from the
    interpolation itself plus 2 e through the rounded difference).  Three levels: 5 + 3 * 5 + 9 * 5 = 65 u m."""
    img, lbl = _volume(3, 1, (23, 20, 27), seed=2)              # white noise: no smoothness to hide an error behind
    S, corner = (12, 12, 10), (6, 3, 9)
    M = A.build_matrix(np.float32([0.3, -0.2, 0.5]), np.float32([1.25, 1.25, 1.25]))
    worst = 0.0
    for flips, k in ((0, 0), (5, 3)):
        sc = A.source_coords(S, corner, flips, k, (0, 1), M, img.shape[1:])
        err = float((A.trilinear_f32(img, sc).double() - _trilinear_f64(img, sc)).abs().max())
        worst = max(worst, err)
        assert err <= 65 * 2.0 ** -24 * float(img.abs().max()), err
    assert worst > 0.0                                          # the comparison is not vacuous: float32 does round here
    # a volume exactly the crop's size: the warped footprint leaves it on every side and clamps
    small = img[:, :12, :12, :10].contiguous()
    sc = A.source_coords(S, (0, 0, 0), 0, 0, (0, 1), M, small.shape[1:])
    assert float(sc.min()) < 0 and all(float(sc[a].max()) > small.shape[1 + a] - 1 for a in range(3))
    err = float((A.trilinear_f32(small, sc).double() - _trilinear_f64(small, sc)).abs().max())
    assert err <= 65 * 2.0 ** -24 * float(small.abs().max()), err


def test_zoom_direction_and_nearest_label():
    """zoom 2 reads half as far from the crop centre (structures twice as large); the label index is floor(src + 0.5)"""
    img, lbl = _volume(1, 1, (16, 16, 16), seed=3)
    ramp = torch.arange(16.0).view(1, 1, 1, 16).expand(1, 16, 16, 16).contiguous()
    S, corner = (8, 8, 8), (4, 4, 4)
    x, _ = A.affine_sample(ramp, lbl, corner, S, 0, 0, (0, 1), A.build_matrix((0, 0, 0), (2.0, 2.0, 2.0)))
    assert torch.equal(x[0, 0, 0], 7.5 + (torch.arange(8.0) - 3.5) / 2)
    x, _ = A.affine_sample(ramp, lbl, (8, 8, 8), S, 0, 0, (0, 1), A.build_matrix((0, 0, 0), (0.5, 0.5, 0.5)))
    assert torch.equal(x[0, 0, 0], (11.5 + (torch.arange(8.0) - 3.5) * 2).clamp(0, 15))     # border padding past the volume
    sc = A.source_coords(S, corner, 0, 0, (0, 1), A.build_matrix((0, 0, 0), (2.0, 2.0, 2.0)), (16, 16, 16))
    _, y = A.affine_sample(img, lbl, corner, S, 0, 0, (0, 1), A.build_matrix((0, 0, 0), (2.0, 2.0, 2.0)))
    n = torch.floor(sc + 0.5).long()
    assert torch.equal(y, lbl[:, n[0], n[1], n[2]].float())


def test_matrix_within_one_ulp_of_an_independent_build():
    """build_matrix (explicit sums, the device's order) against numpy's float64 R0 @ R1 @ R2 @ diag(1 / z) from the same stored
    float32 angles and zooms: within one float32 ulp per entry"""
    g = np.random.default_rng(0)
    for _ in range(200):
        ang = g.uniform(-math.pi, math.pi, 3).astype(np.float32)
        zm = g.uniform(0.5, 2.0, 3).astype(np.float32)
        c, s = np.cos(ang.astype(np.float64)), np.sin(ang.astype(np.float64))
        r0 = np.array([[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]])
        r1 = np.array([[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]])
        r2 = np.array([[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]])
        want = (r0 @ r1 @ r2 @ np.diag(1.0 / zm.astype(np.float64))).astype(np.float32).reshape(9)
        got = A.build_matrix(ang, zm)
        assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))), (ang, zm)
    assert np.array_equal(A.build_matrix((0, 0, 0), (1, 1, 1)), np.eye(3, dtype=np.float32).reshape(9))


def test_replay_is_deterministic_and_leaves_blocks_0_to_2_alone():
    cfg = dict(batch_size=8, seed=77, affine_prob=0.5, rotate_range=(0.5, 0.2, 0.0), zoom_range=(0.7, 1.4), zoom_per_axis=False)
    a, b = A.replay_affine(cfg, 3), A.replay_affine(cfg, 3)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    assert torch.equal(A.replay_affine(cfg, 1, call=2)[0], a[2])
    t = torch.cat(a)
    on = t[:, 0] == 1
    assert 0 < int(on.sum()) < t.shape[0] and bool(((t[:, 0] == 0) | on).all())
    assert torch.equal(t[~on], torch.tensor(A.IDENTITY_ROW).expand(int((~on).sum()), 16))
    assert bool((t[on, 1].abs() <= 0.5).all()) and bool((t[on, 2].abs() <= 0.2).all()) and bool((t[on, 3] == 0).all())
    assert bool((t[on, 4] >= 0.7).all()) and bool((t[on, 4] <= 1.4).all())
    assert torch.equal(t[on, 4], t[on, 5]) and torch.equal(t[on, 4], t[on, 6])
    per = torch.cat(A.replay_affine(dict(cfg, zoom_per_axis=True), 3))
    assert torch.equal(per[:, :5], t[:, :5]) and not torch.equal(per[on, 5], t[on, 5])
    # the words: blocks 3 and 4 are new counters; blocks 0..2 are what augment_ref draws, the params table does not move
    for s in range(3):
        w = A.affine_words(77, 5, s)
        assert w == [R.philox4x64_10((5, s, 3, 0), (77, 0)), R.philox4x64_10((5, s, 4, 0), (77, 0))]
        assert all(blk not in R.sample_words(77, 5, s) for blk in w)
    for r in t[on]:
        assert torch.equal(r[7:], torch.from_numpy(A.build_matrix(r[1:4].numpy(), r[4:7].numpy())))
