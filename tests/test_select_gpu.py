"""The radix select (csrc/select.hip behind kth_value / percentile) against numpy: the value bit-equal to np.partition on the same
array (+-0 compared numerically), the two counts equal to a full sort of the keys (tests/select_ref.py), percentiles within 1e-12 of
np.percentile in float64 (the bound tests/test_metrics_gpu.py holds percentiles to: both sides interpolate the same fp32 order
statistics in double), and VolumeCache.add(scale_percentiles=...).

Kernels: four 8-bit histogram passes, 256 threads per workgroup, one 4096-element chunk per workgroup up to 1024 workgroups (above
4 Mi elements the workgroups stride over the chunks), 16-byte loads when n % 4 == 0 and the array is 16-byte aligned, else one
element per thread; the picks run one bin per thread.  Sizes:
  1, 63, 65         below one wave and around it, scalar loop
  4913              two workgroups, the second partial, scalar loop
  17621             five workgroups, the last partial, scalar loop
  17624             the same with 16-byte loads (n % 4 == 0)
  65936             seventeen workgroups, 16-byte loads, the last partial
  4096 + offset     n % 4 == 0 but the array starts 4 bytes past a 16-byte boundary: the scalar loop
  4207832, 4207833  past 1024 chunks: workgroups 0..3 take a second chunk, the last of them partial; 16-byte loads / scalar loop"""
import numpy as np
import pytest
import torch

from guard import Guard, poison_workspace
from select_ref import kth_ref, partition_value, percentile_ref

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 65, 4913, 17621, 17624, 65936]
_DATA = {}


def data(n, seed=0):
    if (n, seed) not in _DATA:
        _DATA[(n, seed)] = (np.random.default_rng(1000 * seed + n).standard_normal(n) * 100 + 20).astype(np.float32)
    return _DATA[(n, seed)]


def ranks(n):
    return sorted({0, n // 2, n - 1})


def check(pkg, xd, x, r, largest):
    """value and counts of one select on the device array xd (= x) against the references"""
    v, beyond, equal = pkg.topk_loss.select_counts(xd, r, largest=largest)
    got = (float(v), int(beyond), int(equal))
    want = kth_ref(x, r, largest)
    print(f"n {x.size} rank {r} largest {largest}: got {got} want {want}")
    assert np.float32(got[0]) == partition_value(x, r, largest)              # numerically: -0 == +0
    assert got[1:] == want[1:]
    k = pkg.kth_value(xd, r, largest=largest)
    assert k.dim() == 0 and k.dtype == torch.float32 and float(k) == got[0]
    return got


def check_all(pkg, dev, x):
    xd = torch.from_numpy(x).to(dev)
    for r in ranks(x.size):
        for largest in (False, True):
            check(pkg, xd, x, r, largest)


@pytest.mark.parametrize("n", SIZES)
def test_sizes(pkg, dev, n):
    check_all(pkg, dev, data(n))


@pytest.mark.parametrize("n", [1024 * 4096 + 3 * 4096 + 1240, 1024 * 4096 + 3 * 4096 + 1241])
def test_more_chunks_than_workgroups(pkg, dev, n):
    """one sort on the host for all six ranks (the data has neither zeros nor ties across the sign, so the key order is numeric)"""
    x = data(n)
    srt = np.sort(x)
    xd = torch.from_numpy(x).to(dev)
    for r in ranks(n):
        for largest in (False, True):
            want = srt[n - 1 - r] if largest else srt[r]
            below, upto = int(np.searchsorted(srt, want, "left")), int(np.searchsorted(srt, want, "right"))
            v, beyond, equal = pkg.topk_loss.select_counts(xd, r, largest=largest)
            assert (float(v), int(beyond), int(equal)) == (float(want), n - upto if largest else below, upto - below)


def test_unaligned_array(pkg, dev):
    x = data(4096, seed=1)
    buf = torch.zeros(4096 + 4, device=dev)
    xd = buf[1:4097]
    xd.copy_(torch.from_numpy(x))
    assert xd.is_contiguous() and xd.data_ptr() % 16 == 4
    for r in ranks(4096):
        for largest in (False, True):
            check(pkg, xd, x, r, largest)


@pytest.mark.parametrize("n", [4913, 17624])
def test_all_elements_equal(pkg, dev, n):
    x = np.full(n, -3.25, np.float32)
    xd = torch.from_numpy(x).to(dev)
    for r in ranks(n):
        for largest in (False, True):
            assert check(pkg, xd, x, r, largest) == (-3.25, 0, n)


@pytest.mark.parametrize("n", [4913, 17624])
def test_two_values_one_mantissa_bit_apart(pkg, dev, n):
    """only the last pass tells them apart"""
    a = np.float32(1.7)
    b = np.nextafter(a, np.float32(2))
    x = np.where(np.random.default_rng(n).random(n) < 0.4, a, b).astype(np.float32)
    na = int((x == a).sum())
    assert 0 < na < n
    xd = torch.from_numpy(x).to(dev)
    assert check(pkg, xd, x, na - 1, False) == (float(a), 0, na)
    assert check(pkg, xd, x, na, False) == (float(b), na, n - na)
    assert check(pkg, xd, x, 0, True) == (float(b), 0, n - na)
    assert check(pkg, xd, x, n - na, True) == (float(a), n - na, na)


@pytest.mark.parametrize("n", [4913, 17624])
def test_values_that_differ_only_above_bit_21(pkg, dev, n):
    """the low 22 bits are zero everywhere: the last two passes and most of the second see one bin"""
    rng = np.random.default_rng(n + 1)
    bits = (rng.integers(0, 2, n).astype(np.uint32) << 31) | (rng.integers(0, 510, n).astype(np.uint32) << 22)      # exponent < 255
    x = bits.view(np.float32)
    assert np.isfinite(x).all()
    check_all(pkg, dev, x)


def test_mixed_signs_and_special_values(pkg, dev):
    x = data(4913, seed=2).copy() - 20.0
    x[:9] = [-0.0, 0.0, 1e-40, -1e-40, np.inf, -np.inf, 0.0, -0.0, 1.4e-45]
    xd = torch.from_numpy(x).to(dev)
    srt = np.sort(x)
    neg = int((srt < 0).sum())
    for r in (0, 1, neg - 1, neg, neg + 1, neg + 2, neg + 3, neg + 4, neg + 5, 4911, 4912):      # both infinities, across the zeros
        for largest in (False, True):
            check(pkg, xd, x, r, largest)
    # -0 sorts below +0: rank `neg` is the first of the two -0, rank neg + 2 the first of the two +0
    v = pkg.kth_value(xd, neg)
    assert float(v) == 0.0 and bool(torch.signbit(v))
    v = pkg.kth_value(xd, neg + 2)
    assert float(v) == 0.0 and not bool(torch.signbit(v))


@pytest.mark.parametrize("n", [4913, 65936])
def test_rank_on_the_ends_of_a_tie_group(pkg, dev, n):
    x = data(n, seed=3).copy()
    srt = np.sort(x)
    lo, size = n // 3, 37
    val = np.float32((srt[lo - 1] + srt[lo]) / 2)                       # 37 copies of a value between two neighbours
    assert srt[lo - 1] < val < srt[lo]
    x[np.argsort(x)[lo:lo + size]] = val
    xd = torch.from_numpy(x).to(dev)
    assert check(pkg, xd, x, lo, False) == (float(val), lo, size)
    assert check(pkg, xd, x, lo + size - 1, False) == (float(val), lo, size)
    assert check(pkg, xd, x, lo + size, False)[1] == lo + size
    above = n - lo - size
    assert check(pkg, xd, x, above, True) == (float(val), above, size)
    assert check(pkg, xd, x, above + size - 1, True) == (float(val), above, size)


def test_rank_from_device_memory(pkg, dev):
    x = data(17621)
    xd = torch.from_numpy(x).to(dev)
    r = torch.tensor([5], dtype=torch.int32, device=dev)
    first = pkg.kth_value(xd, r)
    r.fill_(12000)
    second = pkg.kth_value(xd, r, largest=True)
    assert float(first) == partition_value(x, 5) and float(second) == partition_value(x, 12000, largest=True)


def test_second_call_on_the_same_scratch(pkg, dev):
    """two calls in a row with different data: the second must not see the first's histograms"""
    a, b = data(17624, seed=4), data(4913, seed=5)
    ad, bd = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    pkg.kth_value(ad, 9000)
    v, beyond, equal = pkg.topk_loss.select_counts(bd, 2000)
    want = kth_ref(b, 2000)
    assert (float(v), int(beyond), int(equal)) == (float(want[0]), want[1], want[2])
    check(pkg, ad, a, 9000, True)


@pytest.mark.parametrize("n", [4913, 17624])
def test_inside_guard_with_poisoned_workspace(pkg, dev, n):
    """the array and the result between red zones, the scratch holding the poison pattern: a histogram or state word that is read
    without having been written by this call gives a wild count"""
    x = data(n, seed=6)
    poison_workspace(pkg.functional, dev)
    with Guard(dev) as gd:
        xd = torch.from_numpy(x).to(dev)
        check(pkg, xd, x, n // 2, False)
        check(pkg, xd, x, 7, True)
        torch.cuda.synchronize()
    assert gd.check() > 0


def _close(got, want):
    got, want = np.asarray(got.cpu(), dtype=np.float64), np.asarray(want, dtype=np.float64)
    print("got", got.ravel().tolist(), "want", want.ravel().tolist())
    return got.shape == want.shape and bool((np.abs(got - want) <= 1e-12 * np.abs(want)).all())


Q = (0, 0.5, 50, 99.5, 100)


@pytest.mark.parametrize("n", SIZES)
def test_percentile_sizes(pkg, dev, n):
    x = data(n, seed=7)
    xd = torch.from_numpy(x).to(dev)
    got = torch.cat([pkg.percentile(xd, Q[:4]), pkg.percentile(xd, Q[4])])
    assert got.dtype == torch.float64 and got.shape == (5,)
    assert _close(got, percentile_ref(x, Q))


def test_percentile_of_a_volume(pkg, dev):
    x = data(96 * 80 * 70, seed=8).reshape(96, 80, 70)
    xd = torch.from_numpy(x).to(dev)
    got = torch.cat([pkg.percentile(xd, Q[:4]), pkg.percentile(xd, Q[4:])])
    assert _close(got, percentile_ref(x, Q))


@pytest.mark.parametrize("shape", [(3, 17, 17, 17), (3, 16, 16, 16)])
def test_percentile_channel_wise(pkg, dev, shape):
    """three channels; with 17^3 elements per channel the second and third start off a 16-byte boundary"""
    x = data(int(np.prod(shape)), seed=9).reshape(shape) * np.array([1.0, -2.0, 0.5], np.float32).reshape(3, 1, 1, 1)
    xd = torch.from_numpy(x).to(dev)
    got = pkg.percentile(xd, (0.5, 50, 99.5), channel_wise=True)
    assert got.shape == (3, 3)
    assert _close(got, np.stack([percentile_ref(x[c], (0.5, 50, 99.5)) for c in range(3)]))
    with pytest.raises(ValueError):
        pkg.percentile(xd, (0.5, 101.0))
    with pytest.raises(ValueError):
        pkg.percentile(xd, (1, 2, 3, 4, 5))


@pytest.mark.parametrize("crop", [False, True])
def test_volume_cache_scale_percentiles(pkg, dev, crop):
    """add(scale_percentiles=(0.5, 99.5, 0, 1)) caches, bit for bit, what add(scale_range=(a_min, a_max, 0, 1)) caches with the
    reference's float32 a_min / a_max (the percentiles of the whole image, before the foreground crop)"""
    rng = np.random.default_rng(21)
    img = (rng.standard_normal((1, 20, 18, 22)) * 300 + 100).astype(np.float32)
    img[:, :3] = -5000.0                                                # a margin below the window: 0 after scaling, so
    img[:, :, :2] = -5000.0                                             # CropForegroundd (image > 0) removes it
    lbl = (rng.random((1, 20, 18, 22)) < 0.3).astype(np.float32)
    a_min, a_max = (float(np.float32(v)) for v in percentile_ref(img, (0.5, 99.5)))
    cache = pkg.VolumeCache(dev)
    xi, xl = torch.from_numpy(img).to(dev), torch.from_numpy(lbl).to(dev)
    i = cache.add(xi, xl, scale_percentiles=(0.5, 99.5, 0.0, 1.0), crop_foreground=crop)
    j = cache.add(xi, xl, scale_range=(a_min, a_max, 0.0, 1.0), crop_foreground=crop)
    assert cache.shapes[i] == cache.shapes[j] and (cache.shapes[i][2:] != (20, 18, 22)) == crop
    assert torch.equal(cache.image(i).view(torch.int32), cache.image(j).view(torch.int32))
    assert torch.equal(cache.label(i), cache.label(j))
    for kw in (dict(scale_percentiles=(0.5, 99.5, 0, 1), scale_range=(0, 1, 0, 1)), dict(scale_percentiles=(60, 40, 0, 1)),
               dict(scale_percentiles=(50, 50, 0, 1)), dict(scale_percentiles=(-1, 99, 0, 1)), dict(scale_percentiles=(1, 100.5, 0, 1))):
        with pytest.raises(ValueError):
            cache.add(xi, xl, **kw)
    assert len(cache) == 2
