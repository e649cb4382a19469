"""Exact-arithmetic parity of the conv, transposed-conv and GEMM kernels (tests/exact_ref.py; the checkers and the case lists are
proven on the CPU by tests/test_exact_cpu.py).  Everything goes through pkg.functional / pkg._capi, as the product path does.

Tier A ("int"): integer operands -- every kernel, in every precision mode, returns the float64 result exactly, a bf16-stored
output its round-to-nearest-even bf16.  Tier B (fractional operands whose products the mode forms exactly): every output element
within (terms + 64) 2^-23 sum|a||b| of the float64 result (+ the half ulp of a bf16 store), for the contractions short enough that
one dropped product breaks that bound (exact_ref.tier_b_ok).  The largest |out - ref| / bound of every tier-B check is appended to
the file UNETR_EXACT_PROFILE names (profiles/exact_parity.txt is such a record); it is never asserted on."""
import ctypes
import os

import pytest
import torch

import exact_ref as R
from exact_ref import cl
from test_exact_cpu import (COLSUM, CONV3, CONV3_DGRAD_FUSED, CONV3_IMAGE, CONV3_MAX_WG, CONV3_WGRAD, CONV3_WGRAD_SMALL, CONV_GENERIC, GEMM,
                            GEMM_BF16, GEMM_BF16_BIG, GEMM_BF16_CFGS, GROUPED_WGRAD, LINEAR_X3, LINEAR_X3_DGRAD, OUTCONV, OUTCONV_DIMS, OUTCONV_IN, TCONV)

pytestmark = pytest.mark.gpu

MODES = [(0, "int"), (1, "int"), (2, "int"), (0, "f32"), (1, "bf16"), (2, "s16"), (2, "one")]
MODE_IDS = [f"prec{p}-{f}" for p, f in MODES]
modes = pytest.mark.parametrize("prec,fam", MODES, ids=MODE_IDS)
_RATIOS = []


def mode_params(cases, terms_of, extra=((),)):
    """(case, *extra, prec, fam) for every mode in which the case is checked: tier A always, tier B where one of the case's
    contractions (their lengths: terms_of(case)) is short enough for the bound (exact_ref.tier_b_ok)"""
    out = []
    for case in cases:
        for ex in extra:
            for prec, fam in MODES:
                if fam == "int" or any(R.tier_b_ok(t, prec) for t in terms_of(case)):
                    out.append(pytest.param(case, *ex, prec, fam, id="-".join([str(case).replace(" ", "")] + [str(v) for v in ex] + [f"prec{prec}", fam])))
    return out


def conv_terms(case):
    B, (D, H, W), cin, cout = case
    return (27 * cin, 27 * cout)


def wgrad_routes(case, prec):
    """the launches UNETR_CONV_C1_OFF / UNETR_X3_WGRAD_TR16 select something in"""
    return ["plain", "parts"] + (["c1_off"] if case[2] == 1 and prec == 1 else []) + (["tr16_off"] if prec == 2 else [])


@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    path = os.environ.get("UNETR_EXACT_PROFILE")
    if path and _RATIOS:
        with open(path, "a") as f:
            for row in _RATIOS:
                f.write("%-34s prec %d %-4s %-34s %-12s max|out-ref|/bound = %.3e\n" % row)


def check(kernel, case, name, prec, fam, out, e, stored, lolo=False, ref=None, S=None, extra_terms=0, terms=None):
    """tier A: exact.  tier B: within the bound, where the contraction is short enough for the bound to mean something; the ratio
    is recorded.  ref / S override the entry's (an epilogue on top of the contraction), extra_terms counts its additions."""
    ref = e["ref"] if ref is None else ref
    S = e["S"] if S is None else S
    terms = e["terms"] if terms is None else terms
    what = f"{kernel} {case} {name} prec {prec} {fam}"
    if fam == "int":
        R.assert_exact(out, ref, stored, what)
    elif R.tier_b_ok(terms, prec):
        ratio = R.assert_within(out, ref, S, terms * (4 if prec == 2 else 1) + extra_terms, stored, lolo, what)
        _RATIOS.append((kernel, prec, fam, str(case).replace(" ", ""), name, ratio))


def act(t, prec, dev):
    """NCDHW float32 -> channels-last feature map on the device in the storage type of the mode (exact: the bf16-mode operands are
    bf16 numbers)"""
    t = cl(t).to(dev)
    return t.bfloat16() if prec == 1 else t


def nc(ref):
    """NCDHW reference -> channels-last"""
    return cl(ref)


def filler(shape, fam, seed):
    """what an accumulating kernel adds to: integers in tier A, randn of the mode's operand format otherwise"""
    return R.operand(fam, "act", shape, seed)


# ================================================================================================================ conv side
@modes
@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("case", CONV_GENERIC, ids=str)
def test_conv_generic(pkg, dev, case, ks, prec, fam):
    """implicit-GEMM family (csrc/gemm_conv.hip): conv_pack + conv_fwd forward and data gradient, conv_wgrad"""
    Fn = pkg.functional
    B, dims3, cin, cout = case
    dims = (B,) + dims3
    o = R.conv_ops(case, fam, ks)
    f, d, g = o["fwd"], o["dgrad"], o["wgrad"]
    y = Fn.conv_fwd(cl(f["x"]).to(dev), cin, Fn.conv_pack(f["w"].to(dev), 0), dims, cin, cout, ks, prec)
    check("conv_fwd", case, f"ks{ks} y", prec, fam, y, f, prec == 1, ref=nc(f["ref"]), S=nc(f["S"]))
    dx = Fn.conv_fwd(cl(d["dy"]).to(dev), cout, Fn.conv_pack(d["w"].to(dev), 1), dims, cout, cin, ks, prec)
    check("conv_fwd(dgrad pack)", case, f"ks{ks} dx", prec, fam, dx, d, prec == 1, ref=nc(d["ref"]), S=nc(d["S"]))
    dw = Fn.conv_wgrad(cl(g["x"]).to(dev), cin, cl(g["dy"]).to(dev), cout, dims, cin, cout, ks, prec)
    check("conv_wgrad", case, f"ks{ks} dw", prec, fam, dw, g, False)


@pytest.mark.parametrize("case,prec,fam", mode_params(CONV3, conv_terms))
def test_conv3(pkg, dev, case, prec, fam):
    """dedicated 3x3x3 kernels (csrc/conv3.hip): forward, data gradient (mode 1), and accumulation into a wider-pitched buffer"""
    Fn = pkg.functional
    B, dims3, cin, cout = case
    dims = (B,) + dims3
    o = R.conv_ops(case, fam)
    f, d = o["fwd"], o["dgrad"]
    y = Fn.conv3(act(f["x"], prec, dev), cin, f["w"].to(dev), dims, prec)
    check("conv3", case, "y", prec, fam, y, f, prec == 1, ref=nc(f["ref"]), S=nc(f["S"]))
    dyd, wd = act(d["dy"], prec, dev), d["w"].to(dev)
    dx = Fn.conv3(dyd, cout, wd, dims, prec, mode=1)
    check("conv3 mode 1", case, "dx", prec, fam, dx, d, prec == 1, ref=nc(d["ref"]), S=nc(d["S"]))
    base = filler((B,) + dims3 + (2 * cin,), fam, 21)
    if prec == 1:
        base = R.bf16_rne(base)
    buf = base.to(dev).to(Fn.act_dtype(prec))
    Fn.conv3(dyd, cout, wd, dims, prec, mode=1, out=buf, ldo=2 * cin, accumulate=True)
    lo = base[..., :cin].double()
    check("conv3 accumulate", case, "dx", prec, fam, buf[..., :cin].contiguous(), d, prec == 1, ref=nc(d["ref"]) + lo, S=nc(d["S"]) + lo.abs(),
          extra_terms=1)
    assert torch.equal(buf[..., cin:].float().cpu(), base[..., cin:])              # the other half of the pitch is not touched


def _fused_and_parts(pkg, dev, case, prec, fam, tag):
    Fn = pkg.functional
    B, dims3, cin, cout = case
    dims = (B,) + dims3
    o = R.conv_ops(case, fam)
    f, f3 = o["fwd"], o["fwd3"]
    image = cin < 8                        # the fp32 image in front of encoder1: fp32 storage in bf16 mode too (x_f32)
    xd = cl(f["x"]).to(dev) if image else act(f["x"], prec, dev)
    wd, w3d = f["w"].to(dev), f3["w"].to(dev)
    # conv3_c1_fwd_kernel<PrecBF16x3> (the single-channel image, taps as the K dimension) forms w_hi x_hi + w_hi x_lo + w_lo x_hi, as its
    # comment in csrc/conv3.hip says: the three-product form, with the lo*lo allowance; its 1x1x1 branch is an fp32 product, without
    lolo = prec == 2 and cin == 1
    r = Fn.conv3_fused(xd, cin, wd, w3d, dims, prec)
    assert r is not None
    c, _, c3, _ = r
    check("conv3_fused" + tag, case, "y", prec, fam, c, f, prec == 1, lolo=lolo, ref=nc(f["ref"]), S=nc(f["S"]))
    check("conv3_fused" + tag, case, "y3", prec, fam, c3, f3, prec == 1, ref=nc(f3["ref"]), S=nc(f3["S"]))
    r = Fn.conv3_parts(xd, cin, wd, w3d, dims, prec)
    assert r is not None
    c, part, c3, part3, rows = r
    check("conv3_parts" + tag, case, "y", prec, fam, c, f, prec == 1, lolo=lolo, ref=nc(f["ref"]), S=nc(f["S"]))
    check("conv3_parts" + tag, case, "y3", prec, fam, c3, f3, prec == 1, ref=nc(f3["ref"]), S=nc(f3["S"]))
    if fam == "int":
        # the statistics rows are summed from the fp32 accumulators.  Every value of an (item, channel) column is an integer times ONE
        # power of two, so while sum|n| of the integers as drawn stays below 2^24 every partial sum is exact and the rows add up (in
        # float64) to the exact sum of y.  Every case of the lists stays below: the check may not skip one.
        plain = R.conv_ops(case, "int", scale=False)
        for p, e, name in ((part, f, "fwd"), (part3, f3, "fwd3")):
            ok = plain[name]["ref"].abs().sum((2, 3, 4)) < 2 ** 24                         # [B, Cout]
            assert bool(ok.all()), f"conv3_parts{tag} {case}: an integer column sum reaches 2^24, the sum column would go unchecked"
            got = p.flatten()[:B * rows * 2 * cout].view(B, rows, 2, cout)[:, :, 0, :].double().sum(1).cpu()   # [B][rows][2][Cout]
            want = e["ref"].sum((2, 3, 4))
            assert torch.equal(got, want), f"conv3_parts{tag} {case} prec {prec} {name}: sum column of the partial rows"


@pytest.mark.parametrize("case,prec,fam", mode_params(CONV3 + CONV3_IMAGE, conv_terms))
def test_conv3_fused_and_parts(pkg, dev, case, prec, fam):
    """residual-block front in one launch (conv3x3x3 + the 1x1x1 conv on the same window), with finalized statistics and with
    partial rows; feature maps and the fp32 image (1 / 4 channels)"""
    _fused_and_parts(pkg, dev, case, prec, fam, "")


@modes
def test_conv3_fused_long_tile_walk(pkg, dev, monkeypatch, prec, fam):
    case, max_wg = CONV3_MAX_WG
    monkeypatch.setenv("UNETR_TEST_MAX_WG", str(max_wg))
    _fused_and_parts(pkg, dev, case, prec, fam, f" max_wg={max_wg}")


@pytest.mark.parametrize("case,prec,fam", mode_params(CONV3_DGRAD_FUSED, conv_terms))
def test_conv3_dgrad_fused(pkg, dev, case, prec, fam):
    """dx = conv3x3x3^T(dc1; w1) + conv1x1x1^T(dc3; w3) in one launch; and the data gradient with the InstanceNorm backward
    statistics in its epilogue (dx only: the statistics are not a contraction)"""
    Fn = pkg.functional
    B, dims3, cin, cout = case
    dims = (B,) + dims3
    o = R.conv_ops(case, fam)
    d, d3, both = o["dgrad"], o["dgrad3"], o["dgrad_sum"]
    dc1, dc3, w1, w3 = act(d["dy"], prec, dev), act(d3["dy"], prec, dev), d["w"].to(dev), d3["w"].to(dev)
    dx = torch.empty((B,) + dims3 + (cin,), device=dev, dtype=Fn.act_dtype(prec))
    assert Fn.conv3_dgrad_fused(dc1, dc3, w1, w3, dx, dims, prec)
    check("conv3_dgrad_fused", case, "dx", prec, fam, dx, both, prec == 1, ref=nc(both["ref"]), S=nc(both["S"]))
    xn = act(filler((B, cin) + dims3, fam, 22), prec, dev)
    stats = torch.stack([torch.zeros(B, cin), torch.ones(B, cin)], -1).to(dev)
    r = Fn.conv3_dgrad_stats(dc1, w1, xn, stats, dims, prec)
    assert r is not None
    check("conv3_dgrad_stats", case, "dx", prec, fam, r[0], d, prec == 1, ref=nc(d["ref"]), S=nc(d["S"]))


def _reduce_rows(pkg, dev, part, n, rows):
    capi = pkg._capi
    dst = torch.empty(n, device=dev)
    arr = (capi.ReduceProblem * 1)()
    arr[0].part, arr[0].dst, arr[0].n, arr[0].rows = part.data_ptr(), dst.data_ptr(), n, rows
    capi.call("unetr_reduce_rows_grouped", arr, 1, torch.cuda.current_stream().cuda_stream)
    return dst


WGRAD_PARAMS = [pytest.param(p.values[0], route, p.values[1], p.values[2], id=p.id + "-" + route)
                for p in mode_params(CONV3_WGRAD + CONV3_WGRAD_SMALL, lambda c: (c[0] * c[1][0] * c[1][1] * c[1][2],))
                for route in wgrad_routes(p.values[0], p.values[1])]


@pytest.mark.parametrize("case,route,prec,fam", WGRAD_PARAMS)
def test_conv3_wgrad(pkg, dev, monkeypatch, case, route, prec, fam):
    """dw of the 3x3x3 conv with dw3 of the 1x1x1 branch from the same pass (feature maps and the image form), on every route: the
    dedicated single-channel kernel off (UNETR_CONV_C1_OFF), the bf16x3 (hi, lo)-image kernel off (UNETR_X3_WGRAD_TR16=0), and partial
    rows + reduce_rows_grouped as the arena takes them.  The fp32 dw of the bf16 mode is held to the fp32 bound, not to a bf16 one."""
    Fn, capi = pkg.functional, pkg._capi
    B, dims3, cin, cout = case
    if route == "c1_off":
        monkeypatch.setenv("UNETR_CONV_C1_OFF", "1")
    monkeypatch.setenv("UNETR_X3_WGRAD_TR16", "0" if route == "tr16_off" else "1")
    dims = (B,) + dims3
    o = R.conv_ops(case, fam)
    g, g3 = o["wgrad"], o["wgrad3"]
    image = cin < 8
    xd = cl(g["x"]).to(dev) if image else act(g["x"], prec, dev)
    dyd, dy3d = act(g["dy"], prec, dev), act(g3["dy"], prec, dev)
    # conv3_wgrad_x3_kernel forms dy_hi x_hi + dy_hi x_lo + dy_lo x_hi (csrc/conv3.hip): the three-product form, with the lo*lo allowance;
    # with UNETR_X3_WGRAD_TR16=0 the mode runs conv3_wgrad_kernel<PrecBF16x3>, four products (PrecBF16x3::mma), no allowance
    lolo = prec == 2 and route != "tr16_off"
    if route == "parts":
        x_f32 = int(prec == 1 and xd.dtype == torch.float32)
        rows = capi.load().unetr_conv3_wgrad_rows(B, *dims3, cin, cout, prec, x_f32, 1)
        assert rows > 0
        n, n3 = 27 * cin * cout, cin * cout
        part = torch.empty(rows * (n + n3), device=dev)
        got = ctypes.c_long(0)
        capi.call("unetr_conv3_wgrad_parts", xd.data_ptr(), cin, dyd.data_ptr(), cout, dy3d.data_ptr(), cout, part.data_ptr(), part.numel() * 4,
                  ctypes.byref(got), B, *dims3, cin, cout, prec, x_f32, torch.cuda.current_stream().cuda_stream)
        gr = got.value
        assert 0 < gr <= rows
        dw = _reduce_rows(pkg, dev, part, n, gr).view(cout, cin, 3, 3, 3)
        dw3 = _reduce_rows(pkg, dev, part[gr * n:], n3, gr).view(cout, cin, 1, 1, 1)
    else:
        dw3 = torch.empty(cout, cin, 1, 1, 1, device=dev)
        dw = Fn.conv3_wgrad(xd, cin, dyd, cout, dims, cin, cout, prec, dy3=dy3d, out3=dw3)
    check(f"conv3_wgrad[{route}]", case, "dw", prec, fam, dw, g, False, lolo=lolo)
    check(f"conv3_wgrad[{route}]", case, "dw3", prec, fam, dw3, g3, False, lolo=lolo)


@modes
@pytest.mark.parametrize("case,rng", TCONV, ids=lambda v: str(v))
def test_tconv(pkg, dev, case, rng, prec, fam):
    """2x2x2 stride-2 transposed conv: the generic family, the bf16 GEMM + pixel-shuffle form (its scatter epilogue writes the voxels),
    the dedicated tconv2 kernels; forward, tconv_bwd, the direct data / weight gradient kernels, and a write into one half of a
    concatenation buffer"""
    Fn = pkg.functional
    B, S, cin, cout = case
    dims = (B, S, S, S)
    o = R.tconv_ops(case, fam, rng if fam == "int" else None)
    f, d, g = o["fwd"], o["dgrad"], o["wgrad"]
    xd, wd = act(f["x"], prec, dev), f["w"].to(dev)
    y, xb = Fn.tconv_fwd(xd, cin, wd, dims, cin, cout, prec)
    assert (xb is not None) == (prec == 1 and cin % 64 == 0 and B * S ** 3 < 8192 and (B * S ** 3) % 8 == 0)
    check("tconv_fwd", case, "y", prec, fam, y, f, prec == 1, ref=nc(f["ref"]), S=nc(f["S"]))
    cat = torch.zeros(B, 2 * S, 2 * S, 2 * S, 2 * cout, device=dev, dtype=xd.dtype)
    Fn.tconv_fwd(xd, cin, wd, dims, cin, cout, prec, out=cat, ldo=2 * cout)
    check("tconv_fwd into concat", case, "y", prec, fam, cat[..., :cout].contiguous(), f, prec == 1, ref=nc(f["ref"]), S=nc(f["S"]))
    assert not cat[..., cout:].view(torch.int16 if prec == 1 else torch.int32).any()            # bit-zero
    dyd, wdd = act(d["dy"], prec, dev), d["w"].to(dev)
    dx = Fn.tconv_dgrad(dyd, cout, wdd, dims, cin, cout, prec)
    check("tconv_dgrad", case, "dx", prec, fam, dx, d, prec == 1, ref=nc(d["ref"]), S=nc(d["S"]))
    xg, dyg = act(g["x"], prec, dev), act(g["dy"], prec, dev)
    dw = Fn.tconv_wgrad(xg, cin, dyg, cout, dims, cin, cout, prec)
    check("tconv_wgrad", case, "dw", prec, fam, dw, g, False)
    # tconv_bwd (what autograd calls) on the weight-gradient operands: dw again, through the form forward chose
    _, xbg = Fn.tconv_fwd(xg, cin, wdd, dims, cin, cout, prec)
    dx2, dw2 = Fn.tconv_bwd(xg, cin, xbg, dyd, cout, wdd, dims, cin, cout, prec, True)
    check("tconv_bwd", case, "dx", prec, fam, dx2, d, prec == 1, ref=nc(d["ref"]), S=nc(d["S"]))
    _, dw3 = Fn.tconv_bwd(xg, cin, xbg, dyg, cout, wdd, dims, cin, cout, prec, False)
    check("tconv_bwd", case, "dw", prec, fam, dw3.view(cin, cout, 2, 2, 2), g, False)


@pytest.mark.parametrize("prec,fam", [(0, "int"), (1, "int"), (0, "f32"), (1, "bf16")], ids=["prec0-int", "prec1-int", "prec0-f32", "prec1-bf16"])
@pytest.mark.parametrize("cin,cout", OUTCONV)
def test_outconv(pkg, dev, cin, cout, prec, fam):
    """1x1x1 out conv with bias (fp32 arithmetic on the storage type of the mode): logits, dx, dw, dbias (a column sum)"""
    Fn = pkg.functional
    B, dims3 = OUTCONV_DIMS
    case = (B, dims3, cin, cout)
    o = R.conv_ops(case, fam, 1)
    f, d, g = o["fwd"], o["dgrad"], o["wgrad"]
    V = dims3[0] * dims3[1] * dims3[2]
    bias = R.operand(fam, "w", (cout,), 31)
    bb = bias.double().view(1, cout, 1, 1, 1)
    y = Fn._outconv_fwd(act(f["x"], prec, dev), cin, f["w"].to(dev), bias.to(dev))
    check("outconv_fwd", case, "logits", prec, fam, y.view(B, cout, *dims3), f, False, ref=f["ref"] + bb, S=f["S"] + bb.abs(), extra_terms=1)
    # backward on (dy, w) of the data-gradient entry and on (x, dy) of the weight-gradient entry
    dx, _, _ = Fn._outconv_bwd(d["dy"].to(dev).contiguous(), act(g["x"], prec, dev), cin, d["w"].to(dev), bias.to(dev))
    check("outconv_bwd", case, "dx", prec, fam, dx, d, prec == 1, ref=nc(d["ref"]), S=nc(d["S"]))
    _, dw, db = Fn._outconv_bwd(g["dy"].to(dev).contiguous(), act(g["x"], prec, dev), cin, d["w"].to(dev), bias.to(dev))
    check("outconv_bwd", case, "dw", prec, fam, dw, g, False)
    dyg = g["dy"].double()
    check("outconv_bwd", case, "dbias", prec, fam, db, g, False, ref=dyg.sum((0, 2, 3, 4)), S=dyg.abs().sum((0, 2, 3, 4)), terms=B * V)


@pytest.mark.parametrize("prec,fam", [(0, "int"), (1, "int"), (0, "f32"), (1, "bf16")], ids=["prec0-int", "prec1-int", "prec0-f32", "prec1-bf16"])
@pytest.mark.parametrize("C,cout", OUTCONV_IN)
def test_outconv_in_bwd_contractions(pkg, dev, C, cout, prec, fam):
    """the fused block end + out conv, backward: dout = W^T dlogits (a pure contraction, stored in the feature-map type) and dbias"""
    Fn = pkg.functional
    B, dims3 = OUTCONV_DIMS
    case = (B, dims3, C, cout)
    o = R.conv_ops(case, fam, 1)
    d = o["dgrad"]
    V = dims3[0] * dims3[1] * dims3[2]
    c2, c3 = act(filler((B, C) + dims3, fam, 41), prec, dev), act(filler((B, C) + dims3, fam, 42), prec, dev)
    stats = torch.stack([torch.zeros(B, C), torch.ones(B, C)], -1).to(dev)
    wo, bo = d["w"].to(dev).view(cout, C).contiguous(), torch.zeros(cout, device=dev)
    dl = d["dy"].to(dev).contiguous()
    dout, _, _, _, db = Fn.outconv_in_bwd(dl, c2, stats, c3, stats.clone(), wo, bo, B, V, C)
    check("outconv_in_bwd", case, "dout", prec, fam, dout, d, prec == 1, ref=nc(d["ref"]), S=nc(d["S"]))
    dyd = d["dy"].double()
    check("outconv_in_bwd", case, "dbias", prec, fam, db, d, False, ref=dyd.sum((0, 2, 3, 4)), S=dyd.abs().sum((0, 2, 3, 4)), terms=B * V)


@pytest.mark.parametrize("prec", [0, 1])
def test_layout_moves_and_row_copies_accumulate_exactly(pkg, dev, prec):
    """to_channels_last, nhwc_to_nchw (plain and accumulating) and copy_rows (plain and accumulating, through pitches) on integers:
    moves are copies, sums of small integers are exact in fp32 and round to nearest even in a bf16 destination"""
    Fn, capi = pkg.functional, pkg._capi
    st = torch.cuda.current_stream().cuda_stream
    B, C, dims3 = 2, 16, (5, 6, 7)
    V = 5 * 6 * 7
    x = R.ints((B, C) + dims3, -300, 300, 1)
    assert torch.equal(Fn.to_channels_last(x.to(dev)).cpu(), cl(x))
    a16 = int(prec == 1)
    xl = cl(x).to(dev).to(Fn.act_dtype(prec))                                        # (bf16 mode: rounded here, the operand from now on)
    xl_ref = xl.float().cpu().double()
    for accumulate in (0, 1):
        y0 = R.ints((B, C, V), -300, 300, 2)
        y = y0.to(dev)
        capi.call("unetr_nhwc_to_nchw", xl.data_ptr(), C, y.data_ptr(), B, C, V, accumulate, a16, st)
        want = xl_ref.view(B, V, C).permute(0, 2, 1) + (y0.double() if accumulate else 0)
        R.assert_exact(y, want.contiguous(), False, f"nhwc_to_nchw accumulate={accumulate}")
    rows, cols, ldy, lda = B * V, 8, 16, C
    for accumulate in (0, 1):
        y0 = R.ints((rows, ldy), -300, 300, 3)
        if prec == 1:
            y0 = R.bf16_rne(y0)
        y = y0.to(dev).to(Fn.act_dtype(prec))
        capi.call("unetr_copy_rows", y.data_ptr(), ldy, xl.data_ptr(), lda, rows, cols, accumulate, a16, st)
        want = y0.double().clone()
        want[:, :cols] = xl_ref.view(rows, C)[:, :cols] + (y0[:, :cols].double() if accumulate else 0)
        R.assert_exact(y, want, prec == 1, f"copy_rows accumulate={accumulate}")


# ================================================================================================================ GEMM side
def _gemm(pkg, A, Bm, C, M, N, K, *, prec, lda, ldb, ldc, a_trans=0, b_trans=0, batch=1, strides=(0, 0, 0), bias=None, res=None, ldr=0, res_mod=0,
          accumulate=0, alpha=1.0, b_x3words=0):
    """unetr_gemm through its descriptor (functional.gemm fixes batch = 1)"""
    capi, Fn = pkg._capi, pkg.functional
    d = capi.GemmDesc()
    d.M, d.N, d.K, d.batch, d.a_trans, d.b_trans = M, N, K, batch, a_trans, b_trans
    d.lda, d.ldb, d.ldc = lda, ldb, ldc
    d.strideA, d.strideB, d.strideC = strides
    d.strideR = 0
    d.bias = bias.data_ptr() if bias is not None else None
    d.res = res.data_ptr() if res is not None else None
    d.ldr, d.res_mod = ldr, res_mod
    d.pre = d.aux = None
    d.ldaux, d.act, d.accumulate, d.alpha, d.prec, d.b_x3words = 0, 0, accumulate, alpha, prec, b_x3words
    ws = Fn.workspace(C.device)
    capi.call("unetr_gemm", ctypes.byref(d), A.data_ptr(), Bm.data_ptr(), C.data_ptr(), ws.data_ptr(), ws.numel() * 4,
              torch.cuda.current_stream().cuda_stream)


@modes
@pytest.mark.parametrize("case", GEMM, ids=str)
def test_gemm_layouts_and_epilogues(pkg, dev, case, prec, fam):
    """unetr_gemm: NT (Linear forward), NN (data gradient), TN (weight gradient), a batch of two, bias + residual rows (res_mod),
    accumulate with alpha = 0.5"""
    M, N, K = case
    o = R.gemm_ops(case, fam)
    f, d, g = o["fwd"], o["dgrad"], o["wgrad"]
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    xd, wd = f["x"].to(dev), f["w"].to(dev)
    y = nan(M, N)
    _gemm(pkg, xd, wd, y, M, N, K, prec=prec, lda=K, ldb=K, ldc=N)
    check("gemm NT", case, "y", prec, fam, y, f, False)
    dx = nan(M, K)
    _gemm(pkg, d["dy"].to(dev), d["w"].to(dev), dx, M, K, N, prec=prec, lda=N, ldb=K, ldc=K, b_trans=1)
    check("gemm NN", case, "dx", prec, fam, dx, d, False)
    dw = nan(N, K)
    _gemm(pkg, g["dy"].to(dev), g["x"].to(dev), dw, N, K, M, prec=prec, lda=N, ldb=K, ldc=K, a_trans=1, b_trans=1)
    check("gemm TN", case, "dw", prec, fam, dw, g, False)
    # batch of two: the second item is the first with the rows of A reversed
    xb = torch.stack([f["x"], f["x"].flip(0)]).to(dev)
    yb = nan(2, M, N)
    _gemm(pkg, xb, wd, yb, M, N, K, prec=prec, lda=K, ldb=K, ldc=N, batch=2, strides=(M * K, 0, M * N))
    check("gemm NT batched", case, "y[0]", prec, fam, yb[0], f, False)
    check("gemm NT batched", case, "y[1]", prec, fam, yb[1], f, False, ref=f["ref"].flip(0), S=f["S"].flip(0))
    # bias + residual rows of period L
    L = M // 3 if M % 3 == 0 else M
    bias, res = R.operand(fam, "w", (N,), 51), R.operand(fam, "act", (L, N), 52)
    _gemm(pkg, xd, wd, y, M, N, K, prec=prec, lda=K, ldb=K, ldc=N, bias=bias.to(dev), res=res.to(dev), ldr=N, res_mod=L)
    add = bias.double() + res.double().repeat(M // L, 1)
    sadd = bias.double().abs() + res.double().abs().repeat(M // L, 1)
    check("gemm NT bias+res", case, "y", prec, fam, y, f, False, ref=f["ref"] + add, S=f["S"] + sadd, extra_terms=2)
    y0 = R.operand(fam, "act", (M, N), 53)
    y = y0.to(dev)
    _gemm(pkg, xd, wd, y, M, N, K, prec=prec, lda=K, ldb=K, ldc=N, accumulate=1, alpha=0.5)
    check("gemm NT accumulate alpha", case, "y", prec, fam, y, f, False, ref=y0.double() + 0.5 * f["ref"], S=y0.double().abs() + 0.5 * f["S"],
          extra_terms=1)


def _gemm_bf16_all(pkg, dev, case, fam, tag, b_kn=True):
    """unetr_gemm_bf16 on bf16-stored operands: C and Cb from one launch, and B read as [K, N]"""
    Fn = pkg.functional
    M, N, K = case
    f = R.gemm_ops(case, fam)["fwd"]
    xd, wd = f["x"].to(dev).bfloat16(), f["w"].to(dev).bfloat16()
    y = torch.full((M, N), float("nan"), device=dev)
    yb = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    Fn.gemm_bf16(xd, wd, M, N, K, C=y, Cb=yb)
    check("gemm_bf16" + tag, case, "C", 1, fam, y, f, False)
    check("gemm_bf16" + tag, case, "Cb", 1, fam, yb, f, True)
    if b_kn and K % 64 == 0 and N % 8 == 0:
        y2 = torch.full((M, N), float("nan"), device=dev)
        Fn.gemm_bf16(xd, wd.t().contiguous(), M, N, K, b_kn=True, C=y2)
        check("gemm_bf16 b_kn" + tag, case, "C", 1, fam, y2, f, False)


BF16_MODES = pytest.mark.parametrize("fam", ["int", "bf16"])


@BF16_MODES
@pytest.mark.parametrize("case", GEMM_BF16, ids=str)
def test_gemm_bf16(pkg, dev, case, fam):
    _gemm_bf16_all(pkg, dev, case, fam, "")


@BF16_MODES
@pytest.mark.parametrize("cfg", GEMM_BF16_CFGS)
def test_gemm_bf16_small_m_tiles(pkg, dev, monkeypatch, cfg, fam):
    monkeypatch.setenv("UNETR_GEMM_CFG", cfg)
    for case in GEMM_BF16:
        _gemm_bf16_all(pkg, dev, case, fam, f" cfg={cfg}", b_kn=cfg not in ("6432", "6496"))


@BF16_MODES
@pytest.mark.parametrize("splits", [2, 3])
def test_gemm_bf16_forced_split_k(pkg, dev, monkeypatch, splits, fam):
    monkeypatch.setenv("UNETR_GEMM_SPLITS", str(splits))
    for case in GEMM_BF16:
        _gemm_bf16_all(pkg, dev, case, fam, f" splits={splits}")


@BF16_MODES
@pytest.mark.parametrize("wn", [2, 3, 4])
def test_gemm_bf16_big_tile(pkg, dev, monkeypatch, wn, fam):
    """the 256 x {128, 192, 256} ping-pong kernel forced on a ragged shape"""
    monkeypatch.setenv("UNETR_GEMM_CFG", "256")
    monkeypatch.setenv("UNETR_GEMM_BIG_WN", str(wn))
    _gemm_bf16_all(pkg, dev, GEMM_BF16_BIG, fam, f" big wn={wn}")


def _split_words(pkg, w):
    """the word shadow [hi | lo << 16] of an fp32 weight, same layout and pitch (unetr_split_words)"""
    words = torch.empty(w.shape, dtype=torch.int32, device=w.device)
    pkg._capi.call("unetr_split_words", w.data_ptr(), words.data_ptr(), w.numel(), torch.cuda.current_stream().cuda_stream)
    return words


@pytest.mark.parametrize("fam", ["int", "s16", "one"])
@pytest.mark.parametrize("dma", ["1", "0"])
@pytest.mark.parametrize("case", LINEAR_X3 + LINEAR_X3_DGRAD, ids=str)
def test_linear_bf16x3(pkg, dev, monkeypatch, case, dma, fam):
    """bf16x3 Linear forward and data gradient through linear_fwd / linear_dgrad and gemm with B read as fp32: the LDS-DMA kernel
    where it takes the shape (contraction length % 32 == 0: every forward here, the data gradients of LINEAR_X3_DGRAD), the generic
    family otherwise and under UNETR_X3_GEMM_DMA=0.  Four products per element, no lo*lo allowance."""
    Fn = pkg.functional
    monkeypatch.setenv("UNETR_X3_GEMM_DMA", dma)
    M, N, K = case
    o = R.gemm_ops(case, fam)
    f, d = o["fwd"], o["dgrad"]
    xd, wd = f["x"].to(dev), f["w"].to(dev)
    check(f"linear_fwd dma={dma}", case, "y", 2, fam, Fn.linear_fwd(xd, wd, None, 2), f, False)
    dyd, wdd = d["dy"].to(dev), d["w"].to(dev)
    check(f"linear_dgrad dma={dma}", case, "dx", 2, fam, Fn.linear_dgrad(dyd, wdd, 2), d, False)


@pytest.mark.parametrize("fam", ["int", "s16", "one"])
@pytest.mark.parametrize("case", LINEAR_X3 + LINEAR_X3_DGRAD, ids=str)
def test_linear_bf16x3_word_shadow(pkg, dev, case, fam):
    """the same GEMMs with the weight read as pre-split words (unetr_split_words; b_x3words = 1: launch_bf16<..., X3 = 2>, the only
    kernel that reads a word shadow).  With b_x3words set the entry point returns "unsupported" instead of taking another kernel, so
    a call that succeeds ran that kernel: the forward on every shape, the data gradient where its contraction length N % 32 == 0."""
    M, N, K = case
    o = R.gemm_ops(case, fam)
    f, d = o["fwd"], o["dgrad"]
    xd, wd = f["x"].to(dev), f["w"].to(dev)
    y = torch.full((M, N), float("nan"), device=dev)
    _gemm(pkg, xd, _split_words(pkg, wd), y, M, N, K, prec=2, lda=K, ldb=K, ldc=N, b_x3words=1)
    check("gemm b_x3words", case, "y", 2, fam, y, f, False)
    dyd, wdd = d["dy"].to(dev), d["w"].to(dev)
    dx = torch.full((M, K), float("nan"), device=dev)
    if N % 32 == 0:
        _gemm(pkg, dyd, _split_words(pkg, wdd), dx, M, K, N, prec=2, lda=N, ldb=K, ldc=K, b_trans=1, b_x3words=1)
        check("gemm b_x3words", case, "dx", 2, fam, dx, d, False)
    else:
        with pytest.raises(RuntimeError, match="unsupported"):
            _gemm(pkg, dyd, _split_words(pkg, wdd), dx, M, K, N, prec=2, lda=N, ldb=K, ldc=K, b_trans=1, b_x3words=1)


@modes
def test_grouped_wgrad(pkg, dev, prec, fam):
    """dW_i = dY_i^T X_i of several problems in one launch: unetr_gemm_grouped_wgrad in the three modes on fp32 storage, and the
    bf16-storage form (bf16 mode)"""
    capi = pkg._capi
    st = torch.cuda.current_stream().cuda_stream
    for bf16_storage in ((False, True) if prec == 1 else (False,)):
        arr = (capi.GroupedProblem * len(GROUPED_WGRAD))()
        keep, outs = [], []
        for i, (M, N, K) in enumerate(GROUPED_WGRAD):
            g = R.gemm_ops((M, N, K), fam)["wgrad"]
            dyd, xd = g["dy"].to(dev), g["x"].to(dev)
            if bf16_storage:
                dyd, xd = dyd.bfloat16(), xd.bfloat16()
            out = torch.full((N, K), float("nan"), device=dev)
            keep += [dyd, xd]
            outs.append((out, g))
            arr[i].dy, arr[i].x, arr[i].dw, arr[i].M, arr[i].N, arr[i].K = dyd.data_ptr(), xd.data_ptr(), out.data_ptr(), M, N, K
        if bf16_storage:
            capi.call("unetr_gemm_bf16_grouped_wgrad", arr, len(GROUPED_WGRAD), st)
        else:
            capi.call("unetr_gemm_grouped_wgrad", arr, len(GROUPED_WGRAD), prec, st)
        for (out, g), case in zip(outs, GROUPED_WGRAD):
            check("gemm_bf16_grouped_wgrad" if bf16_storage else "gemm_grouped_wgrad", case, "dw", prec, fam, out, g, False)


@pytest.mark.parametrize("fam", ["int", "s16", "one"])
def test_grouped_wgrad_bf16x3_stacks(pkg, dev, fam):
    """the bf16x3 weight gradients as the arena runs them: unetr_split_stack_bf16_grouped writes [hi; hi; lo] of dY and [hi; lo; hi]
    of X, the bf16 grouped kernel contracts over the 3 M stacked rows -- hi*hi + hi*lo + lo*hi, the three-product form: checked with
    the lo*lo allowance (include/unetr_hip.h: unetr_split_stack_bf16)"""
    capi = pkg._capi
    st = torch.cuda.current_stream().cuda_stream
    n = len(GROUPED_WGRAD)
    sp, gp = (capi.SplitProblem * (2 * n))(), (capi.GroupedProblem * n)()
    keep, outs = [], []
    for i, (M, N, K) in enumerate(GROUPED_WGRAD):
        g = R.gemm_ops((M, N, K), fam)["wgrad"]
        dyd, xd = g["dy"].to(dev), g["x"].to(dev)
        dys, xs = torch.empty(3 * M, N, dtype=torch.bfloat16, device=dev), torch.empty(3 * M, K, dtype=torch.bfloat16, device=dev)
        out = torch.full((N, K), float("nan"), device=dev)
        for a, (src, dst, cols, second) in zip((sp[2 * i], sp[2 * i + 1]), ((dyd, dys, N, 0), (xd, xs, K, 1))):
            a.src, a.dst, a.rows, a.cols, a.second = src.data_ptr(), dst.data_ptr(), M, cols, second
        gp[i].dy, gp[i].x, gp[i].dw, gp[i].M, gp[i].N, gp[i].K = dys.data_ptr(), xs.data_ptr(), out.data_ptr(), 3 * M, N, K
        keep += [dyd, xd, dys, xs]
        outs.append((out, g))
    capi.call("unetr_split_stack_bf16_grouped", sp, 2 * n, st)
    capi.call("unetr_gemm_bf16_grouped_wgrad", gp, n, st)
    for (out, g), case in zip(outs, GROUPED_WGRAD):
        check("split_stack + gemm_bf16_grouped_wgrad", case, "dw", 2, fam, out, g, False, lolo=True)


@pytest.mark.parametrize("fam", ["int", "f32"])
@pytest.mark.parametrize("M,N", COLSUM)
def test_column_sums(pkg, dev, M, N, fam):
    """colsum (plain and accumulating), colsum_grouped (fp32 and bf16 input) and reduce_rows_grouped: bias-gradient reductions"""
    Fn, capi = pkg.functional, pkg._capi
    st = torch.cuda.current_stream().cuda_stream
    case = (M, N)
    x = R.ints((M, N), -4, 4, 1) if fam == "int" else torch.randn(M, N, generator=torch.Generator().manual_seed(1))
    e = dict(ref=x.double().sum(0), S=x.double().abs().sum(0), terms=M)
    xd = x.to(dev)
    check("colsum", case, "sum", 0, fam, Fn.colsum(xd, M, N, N), e, False)
    o0 = R.operand(fam, "act", (N,), 2)
    out = o0.to(dev)
    ws = Fn.workspace(dev)
    capi.call("unetr_colsum", xd.data_ptr(), N, M, N, out.data_ptr(), 1, ws.data_ptr(), ws.numel() * 4, st)
    check("colsum accumulate", case, "sum", 0, fam, out, e, False, ref=e["ref"] + o0.double(), S=e["S"] + o0.double().abs(), extra_terms=1)
    xb = R.bf16_rne(x)
    eb = dict(ref=xb.double().sum(0), S=xb.double().abs().sum(0), terms=M)
    xbd = xb.to(dev).bfloat16()
    nprob = 2 if N % 8 == 0 else 1                 # (bf16 rows are read as whole 16-byte pieces: N % 8 == 0, the entry point declines others)
    arr = (capi.ColsumProblem * nprob)()
    o1, o2 = torch.full((N,), float("nan"), device=dev), torch.full((N,), float("nan"), device=dev)
    arr[0].x, arr[0].out, arr[0].ld, arr[0].M, arr[0].N, arr[0].x_bf16 = xd.data_ptr(), o1.data_ptr(), N, M, N, 0
    if nprob == 2:
        arr[1].x, arr[1].out, arr[1].ld, arr[1].M, arr[1].N, arr[1].x_bf16 = xbd.data_ptr(), o2.data_ptr(), N, M, N, 1
    capi.call("unetr_colsum_grouped", arr, nprob, st)
    check("colsum_grouped", case, "fp32 rows", 0, fam, o1, e, False)
    if nprob == 2:
        check("colsum_grouped", case, "bf16 rows", 0, fam, o2, eb, False)
    check("reduce_rows_grouped", case, "sum", 0, fam, _reduce_rows(pkg, dev, xd, N, M), e, False)


def _cast_inputs():
    """ties, negatives, zeros, binade edges, and random values over many exponents (a multiple of 8 elements)"""
    gen = torch.Generator().manual_seed(7)
    k = torch.arange(1, 400, dtype=torch.float64)
    ties = torch.cat([k + 0.5, (2 * k + 1) * 2.0 ** -9, 257.0 + 2 * k])
    edge = torch.tensor([2.0 ** e * f for e in (-20, -1, 0, 7, 30) for f in (1 - 2.0 ** -9, 1 - 2.0 ** -10, 1 - 2.0 ** -24, 1.0, 1 + 2.0 ** -9,
                                                                             1 + 2.0 ** -8, 1 + 2.0 ** -23, 1 + 2.0 ** -16 + 2.0 ** -23)], dtype=torch.float64)
    rnd = torch.randn(4096, generator=gen).double() * torch.pow(2.0, torch.randint(-20, 20, (4096,), generator=gen).double())
    v = torch.cat([ties, -ties, edge, -edge, torch.zeros(5, dtype=torch.float64), rnd]).float()
    return v[:v.numel() // 8 * 8].contiguous()


def _u16(t):
    return t.view(torch.int16).to(torch.int32) & 0xFFFF


def test_casts_and_splits_bit_exact(pkg, dev):
    """unetr_cast_bf16, unetr_add_cast_bf16, unetr_split_words, unetr_split_stack_bf16 and its grouped form against integer
    arithmetic on the bit patterns: round to nearest even (hi of the word shadow: truncation, as include/unetr_hip.h documents)"""
    Fn, capi = pkg.functional, pkg._capi
    st = torch.cuda.current_stream().cuda_stream
    v = _cast_inputs()
    n = v.numel()
    vd = v.to(dev)
    want = R.bf16_bits_rne(v).to(torch.int32)
    assert torch.equal(_u16(Fn.cast_bf16(vd).cpu()), want)
    other = torch.roll(v, 3) * 0.5
    s = Fn.add_cast(vd, other.to(dev))
    ssum = v + other                                                                    # one IEEE fp32 addition
    assert torch.equal(s.cpu().view(torch.int32), ssum.view(torch.int32))
    assert torch.equal(_u16(s._unetr_bf16[0].cpu()), R.bf16_bits_rne(ssum).to(torch.int32))
    # word shadow: [hi | lo << 16], hi = truncated, lo = bf16(a - hi)
    words = torch.empty(n, dtype=torch.int32, device=dev)
    capi.call("unetr_split_words", vd.data_ptr(), words.data_ptr(), n, st)
    hi = R._bits(v) >> 16
    lo = R.bf16_bits_rne((v.double() - R.bf16_trunc(v).double()).float())
    assert torch.equal(words.cpu().to(torch.int64) & 0xFFFFFFFF, hi | (lo << 16))
    # stacks: hi = bf16(a) to nearest even, lo = bf16(a - hi); [hi; hi; lo] (second = 0) or [hi; lo; hi] (second = 1)
    rows, cols = n // 8, 8
    hi = R.bf16_bits_rne(v)
    lo = R.bf16_bits_rne((v.double() - R.bf16_rne(v).double()).float())
    outs = {}
    for second in (0, 1):
        dst = torch.zeros(3 * n, dtype=torch.bfloat16, device=dev)
        capi.call("unetr_split_stack_bf16", vd.data_ptr(), dst.data_ptr(), rows, cols, second, st)
        outs[second] = dst
        planes = [hi, lo, hi] if second else [hi, hi, lo]
        assert torch.equal(_u16(dst.cpu()).to(torch.int64), torch.cat(planes)), f"split_stack second={second}"
    arr = (capi.SplitProblem * 2)()
    dsts = [torch.zeros(3 * n, dtype=torch.bfloat16, device=dev) for _ in range(2)]
    for i in range(2):
        arr[i].src, arr[i].dst, arr[i].rows, arr[i].cols, arr[i].second = vd.data_ptr(), dsts[i].data_ptr(), rows, cols, i
    capi.call("unetr_split_stack_bf16_grouped", arr, 2, st)
    for i in range(2):
        assert torch.equal(dsts[i].view(torch.int16), outs[i].view(torch.int16)), f"split_stack grouped second={i}"
