"""Host side of the sliding-window inferer (no GPU): the Gaussian importance map against real separable filtering, the planned
window table against the function's own window enumeration, and argument checking."""
import pytest
import torch

from inference_ref import oracle_window_order, ref_importance_map, ref_sliding_window

# (volume, batch, overlap, sw_batch_size) of tests/test_inference_gpu.py, roi 32^3
CASES = [((48, 48, 48), 2, 0.25, 4), ((40, 40, 40), 1, 0.5, 4), ((48, 48, 48), 1, 0.8, 4), ((40, 48, 56), 1, 0.25, 4),
         ((32, 48, 80), 1, 0.25, 4), ((32, 32, 56), 1, 0.25, 4), ((32, 32, 32), 2, 0.25, 4), ((48, 48, 48), 1, 0.25, 3)]


def _max_rel(a, b):
    return ((a.double() - b.double()).abs() / b.double().abs()).max().item()


@pytest.mark.parametrize("roi,sigma", [((32, 32, 32), 0.125), ((96, 96, 96), 0.125), ((32, 24, 16), 0.125), ((32, 32, 32), 0.05),
                                       ((32, 32, 32), (0.125, 0.25, 0.08))])
def test_gaussian_importance_map_equals_separable_filtering(pkg, roi, sigma):
    got = pkg.inference.importance_map(roi, "gaussian", sigma)
    ref = ref_importance_map(roi, "gaussian", sigma)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(roi)
    rel = _max_rel(got, ref)
    print(f"roi {roi} sigma_scale {sigma}: max relative difference {rel:.3e}, min weight {got.min().item():.3e}")
    assert rel <= 1e-6
    assert got.max().item() == 1.0 and got.min().item() > 0.0
    if sigma == 0.05:                    # the tail is shorter than the window: everything outside it takes the clamp
        assert int((got == got.min()).sum()) > 10000


def test_constant_importance_map_is_all_ones(pkg):
    m = pkg.inference.importance_map((32, 24, 16), "constant")
    assert tuple(m.shape) == (32, 24, 16) and bool((m == 1).all())


@pytest.mark.parametrize("size,batch,overlap,n", CASES)
def test_window_table_lists_the_functions_windows_in_order(pkg, size, batch, overlap, n):
    inf = pkg.inference
    roi = (32, 32, 32)
    starts = inf._dense_patch_starts(size, roi, inf._scan_interval(size, roi, overlap))
    flat = [(b,) + tuple(s) for b in range(batch) for s in starts]
    table, counts = inf.plan_window_table(batch, size, roi, overlap, n)
    rows = (len(flat) + n - 1) // n
    assert table.dtype == torch.int32 and tuple(table.shape) == (rows, pkg._capi.SW_ROW_INTS)
    assert counts == [min(n, len(flat) - r * n) for r in range(rows)] and sum(counts) == len(flat)
    got = []
    for r in range(rows):
        assert int(table[r, 0]) == counts[r] and table[r, 1:4].tolist() == [0, 0, 0]
        slots = table[r, 4:].reshape(-1, 4).tolist()
        got += [tuple(s) for s in slots[:counts[r]]]
        assert all(s == [0, 0, 0, 0] for s in slots[counts[r]:])
    assert got == flat
    # and both agree with the order in which the oracle's loop forwards the windows
    groups = oracle_window_order(batch, size, roi, n, overlap)
    assert [len(g) for g in groups] == counts and [w for g in groups for w in g] == flat


def test_reference_loop_reproduces_the_oracle_in_constant_mode():
    from oracle.unetr_oracle import oracle_sliding_window_inference
    torch.manual_seed(0)
    pred = lambda w: torch.cat([w * 2.0 + 1.0, w * w, -w], 1)
    for size, overlap, n in (((40, 44, 52), 0.25, 4), ((24, 40, 30), 0.5, 3), ((36, 36, 36), 0.8, 4)):
        x = torch.randn(2, 1, *size)
        a = oracle_sliding_window_inference(x, (32, 32, 32), n, pred, overlap=overlap)
        b = ref_sliding_window(x, (32, 32, 32), n, pred, overlap=overlap)
        assert torch.equal(a, b), size


def test_invalid_arguments_raise_what_monai_raises(pkg):
    with pytest.raises(ValueError):                    # BlendMode("nearest")
        pkg.SlidingWindowInferer((32, 32, 32), 4, mode="nearest")
    with pytest.raises(ValueError):
        pkg.inference.importance_map((32, 32, 32), "nearest")
    for overlap in (-0.1, 1.0):
        with pytest.raises(AssertionError):            # "overlap must be >= 0 and < 1."
            pkg.SlidingWindowInferer((32, 32, 32), 4, overlap=overlap)
    with pytest.raises(ValueError):                    # ensure_tuple_rep(sigma_scale, 3)
        pkg.inference.importance_map((32, 32, 32), "gaussian", (0.125, 0.125))
    inferer = pkg.SlidingWindowInferer((32, 32, 32), 4)
    assert inferer.stats["captures"] == 0 and inferer.stats["replays"] == 0
    with pytest.raises(RuntimeError, match="ROCm device"):       # no CPU fallback
        inferer(torch.zeros(1, 1, 32, 32, 32), lambda w: w)
