"""Host reference of the device gradient clipping (csrc/grad_clip.hip): a float64 sum of squares and the fp32 coefficient formula of
torch.nn.utils.clip_grad_norm_.  numpy only; bf16 values come in as the float32 numbers they represent."""
import numpy as np


def f32(x):
    return np.float32(x)


def sumsq64(arrays):
    """sum of squares of every element of `arrays` in float64 (each element widened first: the products are exact)"""
    s = np.float64(0.0)
    for a in arrays:
        a = np.asarray(a, dtype=np.float64).reshape(-1)
        s += np.dot(a, a) if a.size < 2 else np.sum(a * a, dtype=np.float64)
    return s


def norm_f32(arrays, gscale=1.0):
    """float32(float32(gscale) * sqrt(sum64)): what the finalize launch writes as `norm`"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float32(np.float64(np.float32(gscale)) * np.sqrt(sumsq64(arrays)))


def coef_f32(norm, max_norm):
    """the fp32 expression of torch: c = max_norm / (norm + 1e-6), clamped to at most 1; NaN stays NaN"""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        c = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
    if np.isnan(c):
        return c
    return c if c < np.float32(1.0) else np.float32(1.0)


def clip_ref(arrays, max_norm, gscale=1.0):
    """(norm, coef) as float32"""
    n = norm_f32(arrays, gscale)
    return n, coef_f32(n, max_norm)


def ulp_diff(a, b):
    """distance of two finite float32 numbers of the same sign in units of the last place"""
    ia = int(np.float32(a).view(np.int32))
    ib = int(np.float32(b).view(np.int32))
    return abs(ia - ib)
