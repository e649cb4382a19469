"""tests/guard.py catches what it claims -- on CPU tensors only.  Every violation here is made with ordinary in-bounds
indexing of the guarded buffer's own base buffer, so nothing faults."""
import struct

import pytest
import torch
import torch.nn.functional as F

from guard import RED_ZONE, Guard, GuardViolation, holds_pattern, pattern_bits, poison_, poisoned

CPU = torch.device("cpu")
DTYPES = [torch.float32, torch.bfloat16, torch.int32, torch.uint8]


def _base_as(gd, t, k=-1):
    """the base buffer of the k-th guarded allocation, viewed in t's dtype; the payload starts at element RED_ZONE / itemsize"""
    rec = gd.records[k]
    assert rec.base.data_ptr() + RED_ZONE == t.data_ptr()
    return rec.base.view(t.dtype), RED_ZONE // t.dtype.itemsize


def test_patterns_are_nans_with_a_payload():
    f32 = struct.unpack("<f", struct.pack("<I", pattern_bits(torch.float32)))[0]
    assert f32 != f32
    assert poisoned((3,), torch.float32, CPU).isnan().all() and poisoned((3,), torch.bfloat16, CPU).isnan().all()
    assert poisoned((3,), torch.float16, CPU).isnan().all() and poisoned((3,), torch.float64, CPU).isnan().all()
    assert poisoned((3,), torch.int32, CPU).tolist() == [0x5A5A5A5A] * 3 and poisoned((3,), torch.uint8, CPU).tolist() == [0x5A] * 3
    assert poisoned((2,), torch.float32, CPU).view(torch.int32).tolist() == [pattern_bits(torch.float32)] * 2
    assert poisoned((2,), torch.bfloat16, CPU).view(torch.int16).tolist() == [pattern_bits(torch.bfloat16)] * 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_alignment_layout_and_interception(dtype):
    with Guard(CPU) as gd:
        a = torch.empty(5, 7, dtype=dtype)
        b = a.new_empty(3)
        c = torch.empty_like(a)
        d = torch.empty_strided((2, 3), (3, 1), dtype=dtype)
        z = torch.zeros(1000, dtype=dtype)
        f = torch.full((9,), 3, dtype=dtype)
        src = (torch.arange(33) % 7).to(dtype)
        e = src.clone()
    assert len(gd.records) == 8                                   # the seven above + the _to_copy of `src`
    for t in (a, b, c, d, z, f, src, e):
        assert t.is_contiguous() and t.data_ptr() % 256 == 0
    for t in (a, b, c, d):
        assert holds_pattern(t)                                   # empty payloads keep the poison
    assert (z == 0).all() and (f == 3).all() and torch.equal(e, src) and torch.equal(src.long(), torch.arange(33) % 7)
    for rec in gd.records:                                        # red zones and the rounding slack hold the pattern
        assert rec.base.numel() % RED_ZONE == 0 and rec.base.numel() >= 3 * RED_ZONE
        for _, zone in rec.zones():
            assert zone.numel() * dtype.itemsize >= RED_ZONE
    assert gd.check() == 8
    # outside the mode, and for other devices or non-contiguous requests inside it, torch allocates as always
    assert not Guard(CPU).records
    with Guard(torch.device("meta")) as other:
        torch.empty(4)
    assert not other.records
    with Guard(CPU) as gd2:
        torch.empty_strided((2, 3), (1, 2))
        torch.empty(0)
    assert not gd2.records


@pytest.mark.parametrize("dtype", DTYPES)
def test_write_past_the_end_is_reported(dtype):
    with Guard(CPU) as gd:
        keep = torch.empty(4, dtype=dtype)
        y = torch.empty(5, 7, dtype=dtype)
    base, start = _base_as(gd, y)
    y.fill_(1)
    assert gd.check() == 2
    base[start + y.numel()] = 1                                   # one element past the ragged tail
    with pytest.raises(GuardViolation) as e:
        gd.check()
    msg = str(e.value)
    name = str(dtype).replace("torch.", "")
    assert msg.count("\n") == 1 and f"empty [5, 7] {name}: red zone after the buffer" in msg
    assert "first at 0 element(s) past the last element" in msg and "red zone before" not in msg
    assert holds_pattern(keep)


@pytest.mark.parametrize("dtype", DTYPES)
def test_write_before_the_start_is_reported(dtype):
    with Guard(CPU) as gd:
        y = torch.zeros(6, 3, dtype=dtype)
        other = torch.empty(8, dtype=dtype)
    base, start = _base_as(gd, y, 0)
    base[start - 1] = 1
    with pytest.raises(GuardViolation) as e:
        gd.check()
    msg = str(e.value)
    name = str(dtype).replace("torch.", "")
    assert msg.count("\n") == 1 and f"zeros [6, 3] {name}: red zone before the buffer" in msg
    assert "first at 1 element(s) before the first element" in msg and "red zone after" not in msg
    assert holds_pattern(other)


def test_far_edges_of_both_red_zones_are_checked():
    with Guard(CPU) as gd:
        y = torch.empty(10)
    base, start = _base_as(gd, y)
    base[0] = 0.0
    base[-1] = 0.0
    lines = gd.violations()
    assert len(lines) == 2 and f"reaches back {RED_ZONE // 4}" in lines[0]
    slack = (RED_ZONE - 40) // 4 + RED_ZONE // 4                  # the payload's rounding slack belongs to the trailing zone
    assert f"first at {slack - 1} element(s) past the last element" in lines[1]


def test_comparison_is_bit_for_bit():
    """a NaN with another payload in a red zone is a write; isnan() would not see it"""
    with Guard(CPU) as gd:
        y = torch.empty(16)
        yb = torch.empty(16, dtype=torch.bfloat16)
    for t, k in ((y, 0), (yb, 1)):
        base, start = _base_as(gd, t, k)
        base[start + t.numel() + 2] = float("nan")
        assert base.isnan().all()
    lines = gd.violations()
    assert len(lines) == 2 and "[16] float32: red zone after" in lines[0] and "[16] bfloat16: red zone after" in lines[1]
    assert "first at 2 element(s) past" in lines[0] and "bits 0x7fc00000" in lines[0] and "bits 0x7fc0" in lines[1]


def test_unwritten_output_element_reaches_the_result():
    def kernel(x, skip):
        y = torch.empty_like(x)                                   # what every wrapper in functional.py does
        for i in range(x.numel()):
            if i != skip:
                y[i] = 2 * x[i]
        return y

    x = torch.arange(37, dtype=torch.float32)
    with Guard(CPU) as gd:
        good, bad = kernel(x, -1), kernel(x, 36)
    assert good.sum().item() == 2 * x.sum().item()
    assert bad.sum().isnan() and torch.equal(bad[:36], good[:36])
    gd.check()                                                    # nothing was written out of bounds: only the value shows it


def _conv_d(x, w, guarded_plane):
    """a 3-tap "conv" along D of x [D, H, W] with padding 1, in plain torch.  `guarded_plane` = the plane the kernel reads for
    d = -1: zeros in the correct version; in the broken one, the plane in front of x in memory."""
    D = x.shape[0]
    planes = [guarded_plane] + [x[d] for d in range(D)] + [torch.zeros_like(x[0])]
    return torch.stack([w[0] * planes[d] + w[1] * planes[d + 1] + w[2] * planes[d + 2] for d in range(D)])


def test_read_before_a_guarded_input_reaches_the_result():
    xs = torch.randn(4, 5, 6, generator=torch.Generator().manual_seed(0))
    w = torch.tensor([0.25, 0.5, -1.0])
    ref = F.conv1d(xs.permute(1, 2, 0).reshape(30, 1, 4), w.view(1, 1, 3), padding=1).reshape(5, 6, 4).permute(2, 0, 1)
    with Guard(CPU) as gd:
        x = xs.to(CPU, copy=True)                                 # the tests' x.to(dev)
    assert len(gd.records) == 1 and torch.equal(x, xs)
    base, start = _base_as(gd, x)
    plane_before = base[start - 30:start].view(5, 6)              # in bounds of the base buffer, one plane before the input
    good = _conv_d(x, w, torch.zeros(5, 6))
    bad = _conv_d(x, w, plane_before)
    assert torch.allclose(good, ref, atol=1e-6)
    assert bad[0].isnan().all() and torch.equal(bad[1:], good[1:])
    # against ordinary memory -- a zeroed neighbour, which is what padding=1 means -- the same broken conv passes
    assert torch.equal(_conv_d(x, w, torch.zeros(30).view(5, 6)), good)
    gd.check()


def test_poison_helpers_on_strided_views():
    """the pitched-operand tests poison one half of a 2C-wide buffer and read the other"""
    cat = poisoned((3, 4, 8), torch.bfloat16, CPU)
    cat[..., :4] = 1.0
    assert holds_pattern(cat[..., 4:]) and not holds_pattern(cat) and not holds_pattern(cat[..., 3:])
    poison_(cat[..., :4])
    assert holds_pattern(cat)
    cat[1, 2, 5] = float("nan")                                   # another NaN is not the pattern
    assert not holds_pattern(cat[..., 4:])
