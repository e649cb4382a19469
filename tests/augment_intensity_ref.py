"""CPU restatement of RandCropAugment's intensity augmentation (a helper module, not a test file; extends augment_ref).

These semantics are this project's own: nnU-Net's choice of operations, MONAI's formulas, no bit parity
with either.  Per sample, after everything augment_ref / augment_affine_ref restate and on x only: blur, noise, brightness,
contrast, gamma.  What is pinned here:

(i)   intensity_words / draw_intensity_row / replay_intensity: Philox blocks 5, 6, 7 of a sample and the int32 [B, 16] table
      ``aug.intensity`` (float values as their bits).  Blocks 0..4 are not touched.
(ii)  blur_radius / blur_weights / blur: the separable Gaussian with border padding inside the crop, taps and sums in the
      device's order, in float32 or float64.
(iii) philox4x64_10_np, noise_uniforms, noise_field: the counter-based Box-Muller normals; u1 and u2 are float32 values both
      sides compute identically, the rest in the dtype asked for.
(iv)  brightness, contrast, gamma in float32 (numpy: one rounding per operation, nothing fuses) and the float64 chain.
"""
import math
import struct

import numpy as np
import torch

import augment_ref as R

INTENSITY_COLS = 16
NOISE, BLUR, BRIGHTNESS, CONTRAST, GAMMA = 1, 2, 4, 8, 16
F32 = np.float32
_OPS = (("noise_prob", "noise_std"), ("blur_prob", "blur_sigma"), ("brightness_prob", "brightness_range"),
        ("contrast_prob", "contrast_range"), ("gamma_prob", "gamma_range"))


def f32_bits(v):
    """the bits of float32(v) as a signed int32"""
    return struct.unpack("<i", struct.pack("<f", float(v)))[0]


def bits_f32(i):
    return struct.unpack("<f", struct.pack("<i", int(i)))[0]


# ---------------------------------------------------------------- (i) the draws
def intensity_words(seed, call, s):
    """blocks 5, 6, 7 of sample s in call `call` (counter (call, s, j, 0), key (seed, 0)).
    Assignment:  block 5: [0] noise flag, [1] noise std, [2] blur flag, [3] brightness flag
                 block 6: [0..2] sigma of axis 0..2, [3] brightness factor
                 block 7: [0] contrast flag, [1] contrast factor, [2] gamma flag, [3] gamma
    A flag is u01(w) < prob; a value is float32(lo + (hi - lo) * u01(w)), computed in double and rounded once."""
    return [R.philox4x64_10((call, s, j, 0), (seed, 0)) for j in (5, 6, 7)]


def _uniform32(rng, w):
    lo, hi = rng
    return float(F32(lo + (hi - lo) * R.u01(w)))


def intensity_row(noise=None, blur=None, brightness=None, contrast=None, gamma=None, call=0):
    """a table row for apply(): an operation given a value (blur: three sigmas) is flagged, the others hold their neutral value"""
    flags = (NOISE * (noise is not None) | BLUR * (blur is not None) | BRIGHTNESS * (brightness is not None)
             | CONTRAST * (contrast is not None) | GAMMA * (gamma is not None))
    sg = (0.0, 0.0, 0.0) if blur is None else blur
    vals = [0.0 if noise is None else noise, *sg, 1.0 if brightness is None else brightness,
            1.0 if contrast is None else contrast, 1.0 if gamma is None else gamma]
    lo, hi = call & 0xFFFFFFFF, call >> 32
    return [flags, *[f32_bits(v) for v in vals], *[v - (1 << 32) if v >> 31 else v for v in (lo, hi)], 0, 0, 0, 0, 0, 0]


def draw_intensity_row(cfg, seed, call, s):
    """the 16 int32 values of sample s; cfg holds the IntensityAugment's fields"""
    b5, b6, b7 = intensity_words(seed, call, s)
    on = lambda w, name: R.u01(w) < cfg[name]  # noqa: E731
    return intensity_row(
        noise=_uniform32(cfg["noise_std"], b5[1]) if on(b5[0], "noise_prob") else None,
        blur=[_uniform32(cfg["blur_sigma"], b6[a]) for a in range(3)] if on(b5[2], "blur_prob") else None,
        brightness=_uniform32(cfg["brightness_range"], b6[3]) if on(b5[3], "brightness_prob") else None,
        contrast=_uniform32(cfg["contrast_range"], b7[1]) if on(b7[0], "contrast_prob") else None,
        gamma=_uniform32(cfg["gamma_range"], b7[3]) if on(b7[2], "gamma_prob") else None, call=call)


def intensity_config(aug):
    it = aug.intensity_config
    return dict({n: getattr(it, n) for pair in _OPS for n in pair}, batch_size=aug.batch_size, seed=aug.seed)


def replay_intensity(cfg, ncalls, call=0):
    """the [B, 16] int32 tables of `ncalls` calls starting at device call counter `call`"""
    return [torch.tensor([draw_intensity_row(cfg, cfg["seed"], call + n, s) for s in range(cfg["batch_size"])], dtype=torch.int32)
            for n in range(ncalls)]


def row_values(row):
    """(flags, std, (sigma0, sigma1, sigma2), brightness, contrast, gamma, call) of a table row, the floats as Python floats"""
    r = [int(v) for v in row]
    v = [bits_f32(b) for b in r[1:8]]
    return r[0], v[0], tuple(v[1:4]), v[4], v[5], v[6], (r[8] & 0xFFFFFFFF) | (r[9] & 0xFFFFFFFF) << 32


# ---------------------------------------------------------------- (ii) blur
def blur_radius(sigma):
    """R = (int)(fmaxf(4.0f * sigma, 0.5f) + 0.5f) in float32"""
    return int(F32(max(F32(4.0) * F32(sigma), F32(0.5))) + F32(0.5))


def blur_weights(sigma, dtype=F32):
    """w_k = g_k / sum(g), g_k = exp(-(k k) / (2 sigma sigma)) for k = -R .. R, the sum in that order, all in `dtype` from the
    float32 value of sigma"""
    t = dtype
    sg = t(F32(sigma))
    rad = blur_radius(sigma)
    g = [np.exp(-t(k * k) / (t(2.0) * sg * sg)).astype(t) for k in range(-rad, rad + 1)]
    total = t(0.0)
    for v in g:
        total = t(total + v)
    return np.array([t(v / total) for v in g], dtype=t)


def blur(x, sigmas, dtype=F32):
    """x [C, S0, S1, S2]: axes 0, 1, 2 in turn; out[i] = sum_k w_k * in[clamp(i + k, 0, S - 1)] accumulated in order k = -R .. R"""
    out = np.asarray(x).astype(dtype)
    for a in range(3):
        w = blur_weights(sigmas[a], dtype)
        rad = (len(w) - 1) // 2
        n = out.shape[1 + a]
        acc = np.zeros_like(out)
        for k in range(-rad, rad + 1):
            idx = np.clip(np.arange(n) + k, 0, n - 1)
            acc = (acc + w[k + rad] * np.take(out, idx, axis=1 + a)).astype(dtype)
        out = acc
    return out


# ---------------------------------------------------------------- (iii) noise
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _mul64(a, b):
    """(high, low) 64 bits of the 128-bit product of uint64 arrays"""
    al, ah, bl, bh = a & _M32, a >> _S32, b & _M32, b >> _S32
    p0, p1, p2, p3 = al * bl, al * bh, ah * bl, ah * bh
    mid = (p0 >> _S32) + (p1 & _M32) + (p2 & _M32)
    return p3 + (p1 >> _S32) + (p2 >> _S32) + (mid >> _S32), a * b


def philox4x64_10_np(ctr, key):
    """augment_ref.philox4x64_10 on uint64 arrays (ctr: four arrays or scalars that broadcast, key: two ints)"""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) for v in np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) for v in ctr])]
    k0, k1 = int(key[0]) & R.M64, int(key[1]) & R.M64
    a, b = np.full(1, 0xD2E7470EE14C6C93, dtype=np.uint64), np.full(1, 0xCA5A826395121157, dtype=np.uint64)
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B97F4A7C15) & R.M64, (k1 + 0xBB67AE8584CAA73B) & R.M64
        hi0, lo0 = _mul64(a, c[0])
        hi1, lo1 = _mul64(b, c[2])
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
    return c


def noise_uniforms(seed, call, s, c, groups):
    """float32 u1, u2 [groups, 4]: group g is counter (call, s, 16 + c, 1 + g), key (seed, 0); word i gives a = low 32 bits and
    b = high 32 bits, u = ((float)(a >> 8) + 0.5f) * 2**-24 (above 2**23 the sum rounds to even, identically on both sides; never 0)"""
    g = np.arange(groups, dtype=np.uint64)
    w = np.stack(philox4x64_10_np((call, s, 16 + c, g + np.uint64(1)), (seed, 0)), axis=1)
    a, b = (w & _M32), (w >> _S32)
    u = lambda v: ((v >> np.uint64(8)).astype(F32) + F32(0.5)) * F32(2.0 ** -24)  # noqa: E731
    return u(a), u(b)


def noise_field(seed, call, s, c, shape, dtype=np.float64):
    """z [S0, S1, S2]: voxel 8 g + j of the channel's ravel order takes normal j of group g; z_2i = r cos t, z_2i+1 = r sin t with
    r = sqrt(-2 log u1_i), t = 2 pi u2_i (float32: the constant 6.283185307179586f), a trailing partial group the first normals"""
    V = int(np.prod(shape))
    groups = -(-V // 8)
    u1, u2 = noise_uniforms(seed, call, s, c, groups)
    t = dtype
    if t == F32:
        r = np.sqrt(F32(-2.0) * np.log(u1))
        ang = F32(6.283185307179586) * u2
    else:
        r = np.sqrt(-2.0 * np.log(u1.astype(t)))
        ang = 2.0 * math.pi * u2.astype(t)
    z = np.stack([r * np.cos(ang), r * np.sin(ang)], axis=2).astype(t)        # [groups, 4, 2] -> 8 per group
    return z.reshape(-1)[:V].reshape(shape)


# ---------------------------------------------------------------- (iv) the pointwise operations
def channel_stats(x):
    """float32 (mn, mx, mean) of one channel: mean = (float)(float64 sum / V)"""
    x = np.asarray(x, dtype=F32)
    return x.min(), x.max(), F32(x.astype(np.float64).sum() / x.size)


def contrast_f32(x, f):
    """one channel: fminf(fmaxf((x - mean) * f + mean, mn), mx) in float32"""
    x = np.asarray(x, dtype=F32)
    mn, mx, mean = channel_stats(x)
    return np.minimum(np.maximum((x - mean) * F32(f) + mean, mn), mx)


def gamma_base_f32(x):
    """(base, rng, mn): base = (x - mn) / (rng + 1e-7f) in float32"""
    x = np.asarray(x, dtype=F32)
    mn, mx, _ = channel_stats(x)
    rng = F32(mx - mn)
    return (x - mn) / F32(rng + F32(1e-7)), rng, mn


def gamma_f32(x, g):
    base, rng, mn = gamma_base_f32(x)
    return np.power(base, F32(g)) * rng + mn


def gamma_f64(x, g):
    """the comparison of the single-operation test: subtraction and division in float32 (correctly rounded on both sides), the
    power, the multiply and the add in float64"""
    base, rng, mn = gamma_base_f32(x)
    return np.power(base.astype(np.float64), float(F32(g))) * float(rng) + float(mn)


def chain_f64(x, row, seed, s):
    """one sample x [C, S0, S1, S2] (the gather's float32 output) through the flagged operations of `row` in float64: blur,
    noise, brightness, contrast, gamma; statistics per channel on what the preceding operation left"""
    flags, std, sigmas, bright, cf, gm, call = row_values(row)
    out = np.asarray(x).astype(np.float64)
    if flags & BLUR:
        out = blur(out, sigmas, np.float64)
    for c in range(out.shape[0]):
        v = out[c]
        if flags & NOISE:
            v = v + std * noise_field(seed, call, s, c, v.shape)
        if flags & BRIGHTNESS:
            v = v * bright
        if flags & CONTRAST:
            mn, mx, mean = v.min(), v.max(), v.mean()
            v = np.clip((v - mean) * cf + mean, mn, mx)
        if flags & GAMMA:
            mn, mx = v.min(), v.max()
            v = np.power((v - mn) / ((mx - mn) + float(F32(1e-7))), gm) * (mx - mn) + mn
        out[c] = v
    return out
