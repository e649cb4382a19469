"""numpy restatement of the order statistics (kth_value, percentile): a full sort of the keys the radix select orders by.

  key = bits ^ (sign ? 0xFFFFFFFF : 0x80000000)  as an unsigned integer: a total order of every fp32 pattern, -0 below +0.

``kth_ref(x, r, largest)`` -> (value, n_beyond, n_equal): the r-th smallest (largest) element, the number of elements strictly
beyond it on the selected side, and the number of elements with its bits.  ``percentile_ref`` is np.percentile in float64."""
import numpy as np


def keys(x):
    b = np.ascontiguousarray(x, dtype=np.float32).ravel().view(np.uint32)
    return b ^ np.where(b >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def unkey(k):
    k = np.uint32(k)
    b = k ^ np.uint32(0x80000000) if k >> 31 else ~k
    return np.array([b], dtype=np.uint32).view(np.float32)[0]


def kth_ref(x, r, largest=False):
    k = np.sort(keys(x))
    n = k.size
    kv = k[n - 1 - r] if largest else k[r]
    beyond = int((k > kv).sum()) if largest else int((k < kv).sum())
    return unkey(kv), beyond, int((k == kv).sum())


def partition_value(x, r, largest=False):
    """the same statistic by np.partition on the array itself (what the device result is held to, +-0 compared numerically)"""
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    i = x.size - 1 - r if largest else r
    return np.partition(x, i)[i]


def percentile_ref(x, q):
    return np.percentile(np.asarray(x).astype(np.float64).ravel(), q)
