"""Slab-mode 3x3x3 kernels under every dispatch the low-resolution decoder levels can get (csrc/conv3.hip: slab_pick): 1 / 2 / 4
output tiles per workgroup, one or two weight images (one image with several slabs = the image refilled per slab), grids in which a
workgroup walks several tiles -- forced through UNETR_CONV3_SLAB_CFG on volumes small enough for a test, once more under
UNETR_TEST_MAX_WG.  Every entry point that reaches the kernel: plain forward, forward with InstanceNorm rows, with the 1x1x1
branch (formed with the tile when the window has several slabs, after it when it has one), accumulate, the data gradient with
backward-statistics rows, the fused data gradient.

References: float64 conv3d on the CPU from the operands as the kernel sees them (tests/exact_ref.py) -- integer operands with exact
equality, bf16-rounded randn operands within the fp32-addition bound of that module.  Statistics are compared as sums over the
partial rows (how many rows a launch writes is the library's choice).  The previous dispatch ("old") stays reachable for one
purpose: outputs of every other dispatch equal its outputs bit for bit, rows included where both write one row per tile."""
import ctypes

import pytest
import torch

import exact_ref as R
from test_exact_ops_gpu import act, check, filler, nc

pytestmark = pytest.mark.gpu

# (B, (D, H, W), cin, cout).  12 / 24 wide like decoder5 / decoder4, ragged in y and x, a single tile, two full x tiles plus a
# half-empty one; one / two / three slabs of 32 bf16 channels; 16 / 32 / 64 outputs = up to 1 / 2 / 4 tiles per workgroup.
# Batch 2 sits on (4, 12, 40): 9 tiles per item, so under UNETR_TEST_MAX_WG=8 a workgroup's walk crosses the batch boundary.
CASES = [(1, (5, 12, 12), 64, 32), (1, (4, 24, 24), 32, 32), (1, (6, 10, 20), 96, 64), (1, (4, 8, 8), 32, 16), (2, (4, 12, 40), 64, 64)]
# None = the dispatcher's own choice; "ntb,wl"
CFGS = ["old", None, "1,2", "1,1", "2,2", "2,1", "4,1", "4,0"]
MODES = [(1, "int"), (1, "bf16"), (0, "int"), (2, "int")]
LRELU = torch.tensor(0.01, dtype=torch.float32).double().item()


def _rows(part, B, rows, C):
    return part.flatten()[:B * rows * 2 * C].view(B, rows, 2, C).cpu()


def _sum_bound(e, v, n, V):
    """bound on |sum_i fl(v_i n_i) - sum_i vref_i n_i| over the voxels of an (item, channel) column: v carries the elementwise error
    e, every product and every one of the < V + 64 fp32 additions one rounding of 2^-23 relative (exact_ref.U23)"""
    mag = (v.abs() + e) * n.abs()
    return (e * n.abs()).sum((1, 2, 3)) + (V + 66) * R.U23 * mag.sum((1, 2, 3))


def _elem_err(entry, fam, prec):
    """elementwise bound on the fp32 accumulator against the float64 reference: none on integers, exact_ref's otherwise"""
    if fam == "int":
        return torch.zeros_like(entry["ref"])
    return (entry["terms"] * (4 if prec == 2 else 1) + R.EXTRA_ADDS) * R.U23 * entry["S"]


def _check_fwd_rows(part, rows, entry, fam, prec, what):
    """sum and sum of squares over the partial rows against the float64 reference (channels-last [B, D, H, W, C])"""
    ref = nc(entry["ref"])
    B, V, C = ref.shape[0], ref[0, ..., 0].numel(), ref.shape[-1]
    got = _rows(part, B, rows, C).double().sum(1)                  # [B, 2, C]
    e = nc(_elem_err(entry, fam, prec))
    one = torch.ones_like(ref)
    b1 = _sum_bound(e, ref, one, V)
    b2 = _sum_bound(e * (2 * ref.abs() + e), ref * ref, one, V)
    assert bool(((got[:, 0] - ref.sum((1, 2, 3))).abs() <= b1).all()), f"{what}: sum column of the partial rows"
    assert bool(((got[:, 1] - (ref * ref).sum((1, 2, 3))).abs() <= b2).all()), f"{what}: sum-of-squares column of the partial rows"
    if fam == "int":
        # integers times one power of two per column (2^-6 at the least: exact_ref scales items and channels by 2^-3 .. 2^3): every
        # partial sum is exact in fp32 while sum |integer| < 2^24
        ok = ref.abs().sum((1, 2, 3)) * 64 < 2 ** 24
        assert torch.equal(got[:, 0][ok], ref.sum((1, 2, 3))[ok]), f"{what}: integer sum column is not exact"


def _run(pkg, dev, case, prec, fam):
    """every entry point once under the environment as it stands: dict of outputs (tensors on the CPU) and row counts"""
    Fn = pkg.functional
    B, dims3, cin, cout = case
    dims = (B,) + dims3
    o = R.conv_ops(case, fam)
    f, f3, d, d3 = o["fwd"], o["fwd3"], o["dgrad"], o["dgrad3"]
    xd, wd, w3d = act(f["x"], prec, dev), f["w"].to(dev), f3["w"].to(dev)
    out = {}
    out["y"] = Fn.conv3(xd, cin, wd, dims, prec)
    r = Fn.conv3_parts(xd, cin, wd, None, dims, prec)
    assert r is not None
    out["y_st"], out["part_st"], out["rows_st"] = r[0], r[1], r[4]
    r = Fn.conv3_parts(xd, cin, wd, w3d, dims, prec)
    assert r is not None
    out["y_b"], out["part_b"], out["y3_b"], out["part3_b"], out["rows_b"] = r
    dyd, wdd = act(d["dy"], prec, dev), d["w"].to(dev)
    base = filler((B,) + dims3 + (2 * cin,), fam, 21)
    if prec == 1:
        base = R.bf16_rne(base)
    buf = base.to(dev).to(Fn.act_dtype(prec))
    Fn.conv3(dyd, cout, wdd, dims, prec, mode=1, out=buf, ldo=2 * cin, accumulate=True)
    out["acc"], out["acc_base"] = buf, base
    xn = filler((B, cin) + dims3, fam, 22)
    stats = torch.stack([torch.zeros(B, cin), torch.ones(B, cin)], -1).to(dev)
    r = Fn.conv3_dgrad_stats(dyd, wdd, act(xn, prec, dev), stats, dims, prec)
    assert r is not None
    out["dx_st"], out["part_bst"], out["rows_bst"] = r
    out["xn"] = xn
    dx = torch.empty((B,) + dims3 + (cin,), device=dev, dtype=Fn.act_dtype(prec))
    assert Fn.conv3_dgrad_fused(dyd, act(d3["dy"], prec, dev), wdd, d3["w"].to(dev), dx, dims, prec)
    out["dx_f"] = dx
    torch.cuda.synchronize()
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out.items()}


def _check_refs(out, case, prec, fam, tag):
    B, dims3, cin, cout = case
    o = R.conv_ops(case, fam)
    f, f3, d, both = o["fwd"], o["fwd3"], o["dgrad"], o["dgrad_sum"]
    st = prec == 1
    for key, e in (("y", f), ("y_st", f), ("y_b", f), ("y3_b", f3), ("dx_st", d), ("dx_f", both)):
        check("conv3 lowres" + tag, case, key, prec, fam, out[key], e, st, ref=nc(e["ref"]), S=nc(e["S"]))
    lo = out["acc_base"][..., :cin].double()
    check("conv3 lowres" + tag, case, "accumulate", prec, fam, out["acc"][..., :cin].contiguous(), d, st, ref=nc(d["ref"]) + lo,
          S=nc(d["S"]) + lo.abs(), extra_terms=1)
    assert torch.equal(out["acc"][..., cin:].float(), out["acc_base"][..., cin:]), f"{tag}: accumulate touched the other half of the pitch"
    _check_fwd_rows(out["part_st"], out["rows_st"], f, fam, prec, f"{case}{tag} forward rows")
    _check_fwd_rows(out["part_b"], out["rows_b"], f, fam, prec, f"{case}{tag} forward rows (with branch)")
    _check_fwd_rows(out["part3_b"], out["rows_b"], f3, fam, prec, f"{case}{tag} 1x1x1 branch rows")
    # backward statistics: n = xn (mean 0, rstd 1), g = dx * lrelu'(n); columns sum g and sum g n
    ref = nc(d["ref"])
    V = ref[0, ..., 0].numel()
    n = nc(out["xn"].double())
    if st:
        n = R.bf16_rne(n).double()
    slope = torch.where(n > 0, torch.ones_like(n), torch.full_like(n, LRELU))
    g = ref * slope
    e = nc(_elem_err(d, fam, prec)) * slope + 2.0 ** -24 * g.abs()
    got = _rows(out["part_bst"], B, out["rows_bst"], cin).double().sum(1)
    assert bool(((got[:, 0] - g.sum((1, 2, 3))).abs() <= _sum_bound(e, g, torch.ones_like(n), V)).all()), f"{case}{tag}: sum g"
    assert bool(((got[:, 1] - (g * n).sum((1, 2, 3))).abs() <= _sum_bound(e, g, n, V)).all()), f"{case}{tag}: sum g n"


def _tiles(case):
    B, (D, H, W), _, _ = case
    return B * -(-W // 16) * -(-H // 4) * -(-D // 4)


def _check_same_bits(out, old, case, tag):
    """tile geometry and the slab -> tap order of every output element do not depend on the dispatch"""
    for key in ("y", "y_st", "y_b", "y3_b", "acc", "dx_st", "dx_f"):
        assert torch.equal(out[key], old[key]), f"{case}{tag}: {key} differs from the previous dispatch in some bit"
    B, _, cin, cout = case
    for part, rows, C in (("part_st", "rows_st", cout), ("part_b", "rows_b", cout), ("part3_b", "rows_b", cout), ("part_bst", "rows_bst", cin)):
        if out[rows] == old[rows] == _tiles(case):          # one tile per workgroup on both sides: the same row per tile
            assert torch.equal(_rows(out[part], B, out[rows], C), _rows(old[part], B, old[rows], C)), f"{case}{tag}: {part} rows differ"


@pytest.mark.parametrize("prec,fam", MODES, ids=[f"prec{p}-{f}" for p, f in MODES])
@pytest.mark.parametrize("case", CASES, ids=lambda c: str(c).replace(" ", ""))
def test_every_dispatch_of_the_slab_kernels(pkg, dev, monkeypatch, case, prec, fam):
    old = None
    for max_wg in (0, 8):
        for cfg in CFGS:
            monkeypatch.delenv("UNETR_CONV3_SLAB_CFG", raising=False)
            monkeypatch.delenv("UNETR_TEST_MAX_WG", raising=False)
            if cfg:
                monkeypatch.setenv("UNETR_CONV3_SLAB_CFG", cfg)
            if max_wg:
                monkeypatch.setenv("UNETR_TEST_MAX_WG", str(max_wg))
            tag = f" cfg={cfg} max_wg={max_wg}"
            out = _run(pkg, dev, case, prec, fam)
            _check_refs(out, case, prec, fam, tag)
            if old is None:
                old = out                      # "old", every workgroup count allowed: the baseline of the bit comparison
            elif cfg != "4,0":                 # (weights from L2 walk the taps in another order: same values, not the same bits)
                _check_same_bits(out, old, case, tag)


def test_forced_forms_are_the_forms_that_run(pkg, monkeypatch):
    """the hook reaches what the test above believes it reaches (the query reports the launch's own choice)"""
    lib = pkg._capi.load()
    o = (ctypes.c_int * 6)()
    want = {"1,2": (1, 2), "1,1": (1, 1), "2,2": (2, 2), "2,1": (2, 1), "4,1": (4, 1), "4,0": (4, 0)}
    for cfg, (ntb, wl) in want.items():
        monkeypatch.setenv("UNETR_CONV3_SLAB_CFG", cfg)
        assert lib.unetr_conv3_slab_dispatch(1, 6, 10, 20, 96, 64, 1, 2, o) == 0
        assert (o[0], o[1]) == (ntb, wl), cfg
    monkeypatch.setenv("UNETR_CONV3_SLAB_CFG", "4,1")
    monkeypatch.setenv("UNETR_TEST_MAX_WG", "8")
    assert lib.unetr_conv3_slab_dispatch(2, 4, 12, 40, 64, 64, 1, 1, o) == 0
    assert (o[0], o[2], o[3]) == (4, 8, 1)                 # 18 tiles on 8 workgroups: walks of 2 and 3 tiles
