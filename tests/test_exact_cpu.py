"""The exact-arithmetic checkers can fail, and the inputs are what they claim to be (tests/exact_ref.py).

* every listed mutation of a reference -- a zeroed tap at a boundary voxel, two swapped output channels, a window shifted by
  one voxel along W, a truncating bf16 store, a dropped hi*lo cross term, a halved last K element -- is rejected by the checker
  of its tier, for every operand family;
* the case lists of tests/test_exact_ops_gpu.py (defined HERE, imported there) satisfy the conditions the tiers rest on:
  S.max() < 2^20 in the integer tier, bf16-stored cases in which a truncating store shows, exact ties on both sides, and a bounded
  tier in which ONE dropped product of median size breaks the bound in at least half of the outputs;
* bf16_rne is torch's cast, and the 16-significant-bit operands split exactly under both hi rules."""
import pytest
import torch

import exact_ref as R

# ---------------------------------------------------------------------------------------------------------------- case lists
# conv side: (B, (D, H, W), cin, cout)
CONV_GENERIC = [(1, (5, 6, 7), 8, 16), (1, (4, 4, 4), 64, 32), (1, (6, 5, 4), 4, 16)]          # conv_pack / conv_fwd / conv_wgrad, KS 1 and 3
CONV3 = [(1, (9, 7, 19), 16, 16), (2, (6, 10, 20), 32, 16), (1, (5, 6, 7), 16, 32), (2, (4, 4, 16), 256, 128)]
CONV3_IMAGE = [(1, (9, 7, 19), 1, 16), (1, (10, 9, 33), 4, 16)]                                   # fp32 image in front of encoder1 (x_f32)
CONV3_MAX_WG = ((2, (6, 10, 20), 32, 16), 8)                                                      # UNETR_TEST_MAX_WG: the long tile walk
CONV3_DGRAD_FUSED = [(1, (9, 7, 19), 16, 16), (1, (10, 9, 33), 48, 16)]
CONV3_WGRAD = [(2, (8, 8, 16), 16, 16), (1, (9, 7, 19), 32, 16), (2, (9, 7, 19), 1, 16)]
# 210 / 756 voxels: weight-gradient contractions short enough for the bounded tier in bf16x3 mode; the second is the image form
CONV3_WGRAD_SMALL = [(1, (5, 6, 7), 16, 32), (1, (9, 7, 12), 1, 16)]
# transposed conv: (B, S, cin, cout); the third entry = integer range of the tier-A operands
TCONV = [((1, 5, 32, 16), None), ((2, 6, 768, 32), 1), ((1, 17, 16, 8), None), ((1, 13, 64, 32), None), ((1, 14, 16, 64), None)]
OUTCONV = [(16, 4), (16, 14), (32, 3)]                # (cin, cout)
OUTCONV_DIMS = (1, (6, 6, 6))                         # 216 voxels (the weight / bias gradients contract over them)
OUTCONV_IN = [(16, 4), (16, 2)]                       # what the fused block-end + out conv takes: C <= 16, Cout <= 4
# GEMM side: (M, N, K)
GEMM = [(37, 50, 44), (33, 64, 32), (300, 32, 256)]
GEMM_BF16 = [(37, 56, 64), (130, 200, 192)]
GEMM_BF16_BIG = (1030, 520, 192)
GEMM_BF16_CFGS = ["6464", "6432", "3264", "64128", "6496"]
LINEAR_X3 = [(430, 772, 96), (50, 200, 160)]
LINEAR_X3_DGRAD = [(430, 768, 96), (50, 192, 160)]    # data gradients the LDS-DMA kernel takes: contraction length N % 32 == 0, K >= 64
GROUPED_WGRAD = [(216, 200, 136), (64, 8, 8), (432, 768, 768)]
COLSUM = [(35, 9), (16, 300), (1000, 64)]             # (rows, columns)

# which outputs of a conv-side case are stored as bf16 in bf16 mode (feature maps and their gradients; weight gradients are fp32)
BF16_STORED = ("fwd", "fwd3", "dgrad", "dgrad3", "dgrad_sum")


def all_cases():
    """(side, label, builder(fam, scale)) of every case the GPU file runs through a contraction"""
    out = []
    for c in CONV_GENERIC:
        for ks in (1, 3):
            out.append(("conv", f"conv{ks} {c}", lambda fam, scale=True, c=c, ks=ks: R.conv_ops(c, fam, ks, scale=scale)))
    for c in sorted(set(CONV3 + CONV3_IMAGE + CONV3_DGRAD_FUSED + CONV3_WGRAD + CONV3_WGRAD_SMALL + [CONV3_MAX_WG[0]])):
        out.append(("conv", f"conv3 {c}", lambda fam, scale=True, c=c: R.conv_ops(c, fam, scale=scale)))
    for cin, cout in sorted(set(OUTCONV + OUTCONV_IN)):
        c = OUTCONV_DIMS + (cin, cout)
        out.append(("conv", f"outconv {c}", lambda fam, scale=True, c=c: R.conv_ops(c, fam, 1, scale=scale)))
    for c, rng in TCONV:
        out.append(("conv", f"tconv {c}", lambda fam, scale=True, c=c, rng=rng: R.tconv_ops(c, fam, rng if fam == "int" else None, scale=scale)))
    for c in sorted(set(GEMM + GEMM_BF16 + [GEMM_BF16_BIG] + LINEAR_X3 + LINEAR_X3_DGRAD + GROUPED_WGRAD)):
        out.append(("gemm", f"gemm {c}", lambda fam, scale=True, c=c: R.gemm_ops(c, fam, scale=scale)))
    return out


ALL = all_cases()
IDS = [label for _, label, _ in ALL]


# ------------------------------------------------------------------------------------------------ helpers: bits and splits
def test_bf16_rne_is_torchs_cast():
    gen = torch.Generator().manual_seed(0)
    t = torch.randn(1 << 16, generator=gen) * torch.pow(2.0, torch.randint(-20, 20, (1 << 16,), generator=gen).float())
    k = torch.arange(1, 600, dtype=torch.float64)
    ties = torch.cat([k + 0.5, (2 * k + 1) * 2.0 ** -9, 257.0 + 2 * k])                       # half way between two bf16 numbers
    edge = torch.tensor([2.0 ** e * f for e in (-10, 0, 7, 20) for f in (1 - 2.0 ** -9, 1 - 2.0 ** -10, 1 - 2.0 ** -24, 1.0, 1 + 2.0 ** -9,
                                                                            1 + 2.0 ** -8, 1 + 2.0 ** -23)], dtype=torch.float64)
    for v in (t.double(), ties, -ties, edge, -edge, torch.zeros(3, dtype=torch.float64)):
        assert torch.equal(R.bf16_rne(v), v.float().bfloat16().float())
    assert R.has_tie(torch.tensor([3.0, 257.0])) and not R.has_tie(torch.tensor([3.0, 258.0, 255.0]))
    assert R.bf16_rne(torch.tensor([257.0, 259.0], dtype=torch.float64)).tolist() == [256.0, 260.0]        # ties go to the even neighbour
    assert R.bf16_trunc(torch.tensor([259.0, -259.0], dtype=torch.float64)).tolist() == [258.0, -258.0]


def test_sig16_and_one_sided_split_exactly():
    gen = torch.Generator().manual_seed(1)
    t = torch.randn(1 << 20, generator=gen) * torch.pow(2.0, torch.randint(-6, 7, (1 << 20,), generator=gen).float())
    s = R.sig16(t)
    assert ((s.double() - t.double()).abs() <= t.double().abs() * 2.0 ** -16).all()
    assert ((R._bits(s) & 0xFF) == 0).all()
    for trunc, worst in ((False, 2.0 ** -8), (True, 2.0 ** -7)):
        hi, lo = R.split_hi_lo(s, trunc)
        assert torch.equal(hi + lo, s.double())                                   # the pair carries the value exactly
        assert ((lo.abs() / s.double().abs()).max() <= worst)
        assert (lo.abs() * lo.abs() <= 2.0 ** -14 * s.double().abs() ** 2).all()
    o = R.one_sided(t)
    (hr, lr), (ht, lt) = R.split_hi_lo(o, False), R.split_hi_lo(o, True)
    assert torch.equal(hr, ht) and torch.equal(lr, lt) and torch.equal(hr + lr, o.double())
    assert (lr > 0).all() and (lr / o.double() >= 2.0 ** -10 * 1.9).all()         # 127/256 of a bf16 ulp: within 2x of its maximum 2^-8
    assert (R.sig16(o) == o).all()


def test_pow2_rows_and_ints():
    x = R.ints((5, 7), -4, 4, 0)
    assert x.dtype == torch.float32 and (x == x.round()).all() and x.min() == -4 and x.max() == 4
    y = R.pow2_rows(R.sig16(torch.randn(5, 7)), -6, 6, 3, axis=1)
    assert (R.sig16(y) == y).all()
    z = R.pow2_rows(torch.ones(5, 7), -6, 6, 3, axis=1)
    assert (z[0:1] == z).all() and len(set(z[0].tolist())) > 2 and (torch.log2(z) == torch.log2(z).round()).all()


# ------------------------------------------------------------------------------------------------ the checkers can fail
def _rejects(fn):
    with pytest.raises(AssertionError, match="elements off"):
        fn()


def _as_out(t64, stored):
    return R.bf16_rne(t64).bfloat16() if stored else t64.float()


def _check(fam, out64, e, stored, terms_mul=1, lolo=False, rounded=True):
    """run the checker of the family's tier on a float64 'kernel result' (stored as the kernel would store it)"""
    out = _as_out(out64, stored) if rounded else R.bf16_trunc(out64).bfloat16()
    if fam == "int":
        R.assert_exact(out, e["ref"], stored)
    else:
        R.assert_within(out, e["ref"], e["S"], e["terms"] * terms_mul, stored, lolo)


FAMS = ["int", "f32", "bf16", "s16", "one"]
MUT_CONV = (1, (5, 6, 7), 16, 32)
MUT_TCONV = (1, 5, 32, 16)
MUT_GEMM = (37, 50, 44)


def _conv_mutants(e):
    """wrong conv forwards, float64: (name, result)"""
    x, w, ref = e["x"].double(), e["w"].double(), e["ref"]
    cout, cin = w.shape[:2]
    # a tap dropped at ONE boundary voxel: output (0, co, 0, 1, W-1) loses w[co, ci, 1, 1, 0] * x[0, ci, 0, 1, W-2], picked non-zero
    W = x.shape[-1]
    prod = w[:, :, 1, 1, 0] * x[0, :, 0, 1, W - 2]
    co, ci = [int(v) for v in torch.unravel_index(prod.abs().argmax(), prod.shape)]
    assert prod[co, ci] != 0
    tap = ref.clone()
    tap[0, co, 0, 1, W - 1] -= prod[co, ci]
    swap = ref.clone()
    swap[:, [0, 1]] = ref[:, [1, 0]]
    shift = R.conv_fwd(torch.roll(x, 1, dims=-1), w)
    wl = w.clone()
    wl[:, cin - 1, -1, -1, -1] *= 0.5                                  # the last K element (last channel of the last tap) at half weight
    return [("tap", tap), ("swap", swap), ("shift", shift), ("tail", R.conv_fwd(x, wl))]


def _gemm_mutants(e):
    x, w, ref = e["x"].double(), e["w"].double(), e["ref"]
    prod = x[:, -1:] * w[:, -1:].t()
    one = ref.clone()                                                 # one product dropped at a corner of the output: its largest
    k = int((x[-1] * w[-1]).abs().argmax())
    assert x[-1, k] * w[-1, k] != 0
    one[-1, -1] -= x[-1, k] * w[-1, k]
    swap = ref.clone()
    swap[:, [0, 1]] = ref[:, [1, 0]]
    shift = torch.roll(x, 1, dims=1) @ w.t()
    return [("tap", one), ("swap", swap), ("shift", shift), ("tail", ref - 0.5 * prod)]


def _tconv_mutants(e):
    x, w, ref = e["x"].double(), e["w"].double(), e["ref"]
    swap = ref.clone()
    swap[:, [0, 1]] = ref[:, [1, 0]]
    wl = w.clone()
    wl[-1] *= 0.5
    tap = ref.clone()
    prod = x[0, :, 0, 0, -1, None] * w[:, :, 0, 0, 1]                  # [cin, cout]: the products of output voxel (0, 0, 2S-1)
    ci, co = [int(v) for v in torch.unravel_index(prod.abs().argmax(), prod.shape)]
    tap[0, co, 0, 0, -1] -= prod[ci, co]
    return [("tap", tap), ("swap", swap), ("shift", R.tconv_fwd(torch.roll(x, 1, dims=-1), w)), ("tail", R.tconv_fwd(x, wl))]


@pytest.mark.parametrize("stored", [False, True])
@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("op", ["conv", "tconv", "gemm"])
def test_mutations_are_rejected(op, fam, stored):
    """the unmutated reference passes (stored with round-to-nearest where the output is bf16), every mutant is rejected"""
    if op == "conv":
        e, muts = R.conv_ops(MUT_CONV, fam)["fwd"], _conv_mutants
    elif op == "tconv":
        e, muts = R.tconv_ops(MUT_TCONV, fam)["fwd"], _tconv_mutants
    else:
        e, muts = R.gemm_ops(MUT_GEMM, fam)["fwd"], _gemm_mutants
    mul = 4 if fam in ("s16", "one") else 1
    _check(fam, e["ref"], e, stored, mul)
    for name, bad in muts(e):
        assert not torch.equal(bad, e["ref"]), name
        with pytest.raises(AssertionError, match="elements off") as err:
            _check(fam, bad, e, stored, mul)
        msg = str(err.value)                      # the count, and the index, value and reference of the worst element
        assert " of %d elements off" % e["ref"].numel() in msg and "worst at (" in msg and "got " in msg and "reference " in msg, name
        if name == "tap":
            assert ": 1 of " in msg               # exactly the one voxel that lost its tap


@pytest.mark.parametrize("fam", ["bf16", "f32", "s16", "one"])
@pytest.mark.parametrize("op", ["conv", "tconv", "gemm"])
def test_truncating_store_is_rejected(op, fam):
    e = {"conv": lambda: R.conv_ops(MUT_CONV, fam), "tconv": lambda: R.tconv_ops(MUT_TCONV, fam), "gemm": lambda: R.gemm_ops(MUT_GEMM, fam)}[op]()["fwd"]
    mul = 4 if fam in ("s16", "one") else 1
    _check(fam, e["ref"], e, True, mul)
    _rejects(lambda: _check(fam, e["ref"], e, True, mul, rounded=False))


def test_truncating_store_is_rejected_on_integers():
    """tier A: outputs above 256 are inexact in bf16 (conv 256 -> 128, K = 6912: most of them), and exact ties exist"""
    e = R.conv_ops(CONV3[3], "int")["fwd"]
    _check("int", e["ref"], e, True)
    _rejects(lambda: _check("int", e["ref"], e, True, rounded=False))
    assert R.has_tie(e["ref"])
    b = R._bits(e["ref"].float())                                     # ties rounded away from zero instead of to even
    up = R._from_bits(((b + 0x8000) >> 16) << 16)
    assert ((up == R.bf16_rne(e["ref"])) | ((b & 0xFFFF) == 0x8000)).all()    # (differs from round-to-nearest-even on ties only)
    _rejects(lambda: R.assert_exact(up.bfloat16(), e["ref"], True))


@pytest.mark.parametrize("trunc_hi", [False, True])
@pytest.mark.parametrize("fam,op", [("s16", "gemm"), ("s16", "conv1"), ("one", "gemm"), ("one", "conv"), ("one", "tconv")])
def test_dropped_cross_term_is_rejected(fam, op, trunc_hi):
    """bf16x3 with a hi*lo term missing, emulated in float64 on operands that split exactly: a_hi b_hi + a_lo b_hi + a_lo b_lo (the
    a_hi b_lo products dropped).  Random signs: K <= 256 (the term averages out as sqrt(K), the allowance grows as K); the one-sided
    family at any K.  The complete four-product sum passes without the lo*lo allowance, the three-product form with it."""
    if op == "gemm":
        e, fn = R.gemm_ops(MUT_GEMM, fam)["fwd"], lambda a, b: a @ b.t()              # K = 44
    elif op == "conv1":
        e, fn = R.conv_ops(CONV_GENERIC[1], fam, 1)["fwd"], R.conv_fwd                 # 1x1x1, K = 64
    elif op == "conv":
        e, fn = R.conv_ops(MUT_CONV, fam)["fwd"], R.conv_fwd                           # K = 432
    else:
        e, fn = R.tconv_ops(MUT_TCONV, fam)["fwd"], R.tconv_fwd
    assert fam == "one" or e["terms"] <= 256
    (ah, al), (bh, bl) = R.split_hi_lo(e["x"], trunc_hi), R.split_hi_lo(e["w"], trunc_hi)
    four = fn(ah, bh) + fn(ah, bl) + fn(al, bh) + fn(al, bl)
    assert torch.equal(four, e["ref"]) or (four - e["ref"]).abs().max() <= 1e-12 * e["S"].max()
    for stored in (False, True):
        _check(fam, four, e, stored, 4)
        _check(fam, four - fn(al, bl), e, stored, 4, lolo=True)                        # the documented three-product form
        _rejects(lambda: _check(fam, four - fn(ah, bl), e, stored, 4))
        _rejects(lambda: _check(fam, four - fn(ah, bl), e, stored, 4, lolo=True))
        _rejects(lambda: _check(fam, four - fn(al, bh), e, stored, 4, lolo=True))
    # (a missing lo*lo term alone, <= 2^-16 S, is NOT told apart from accumulation error once 4 K 2^-23 exceeds it, K >= 32: the
    # lolo allowance only matters for the shortest contractions)


# ------------------------------------------------------------------------------------- conditions on the GPU file's case lists
@pytest.mark.parametrize("side,label,build", ALL, ids=IDS)
def test_integer_tier_stays_exact(side, label, build):
    """every partial sum of every output stays far below 2^24: S.max() < 2^20 on the integers as drawn, the references are integers;
    with the power-of-two channel scaling the GPU file runs them with, the references are still fp32 numbers and the operands still
    bf16 numbers"""
    for name, e in build("int", scale=False).items():
        assert float(e["S"].max()) < R.INT_S_CAP, (label, name, float(e["S"].max()))
        assert torch.equal(e["ref"], e["ref"].round()) and torch.equal(e["ref"].float().double(), e["ref"])
    for name, e in build("int").items():
        assert torch.equal(e["ref"].float().double(), e["ref"]), (label, name)
        for k, v in e.items():
            if k not in ("ref", "S", "terms"):
                assert torch.equal(R.bf16_rne(v), v), (label, name, k)
        plain = build("int", scale=False)[name]["ref"]
        nz = plain != 0
        ratio = (e["ref"][nz] / plain[nz]).abs()
        assert torch.equal(torch.log2(ratio), torch.log2(ratio).round()) and ratio.max() <= 4.0 ** R.INT_SCALE, (label, name)


def _truncation_shows(ref):
    return float((R.bf16_trunc(ref) != R.bf16_rne(ref)).double().mean())


def stored_outputs(side, label):
    """the outputs of a case that some kernel stores as bf16 in bf16 mode: conv-side feature maps and their gradients, and the Cb
    output of gemm_bf16 (forward entry of its cases)"""
    if side == "conv":
        return BF16_STORED
    return ("fwd",) if any(label == f"gemm {c}" for c in GEMM_BF16 + [GEMM_BF16_BIG]) else ()


STORED_CASES = [c for c in ALL if stored_outputs(c[0], c[1])]


@pytest.mark.parametrize("side,label,build", STORED_CASES, ids=[c[1] for c in STORED_CASES])
def test_truncating_store_shows_in_bf16_stored_cases(side, label, build):
    """a truncating store has to move at least 1 % of every bf16-stored output.  Where the case runs in tier B (every contraction
    short enough for it) the bf16-rounded fractional operands must show it: small integer sums (K = 32 at |x| <= 4, |w| <= 3) are
    bf16 numbers themselves, no choice of integers in the ranges of tier A makes 1 % of them inexact.  The contractions too long for
    tier B (K = 6912) run on integers only and must show it there."""
    for name, e in build("bf16").items():
        if name not in stored_outputs(side, label):
            continue
        if R.tier_b_ok(e["terms"], 1):
            frac = _truncation_shows(e["ref"])
        else:
            frac = _truncation_shows(build("int")[name]["ref"])
        assert frac >= 0.01, (label, name, frac)


def test_exact_ties_on_both_sides():
    conv = [R.conv_ops(c, "int")[k]["ref"] for c in CONV3 for k in ("fwd", "dgrad")]
    gemm = [R.gemm_ops(c, "int")[k]["ref"] for c in GEMM_BF16 + [GEMM_BF16_BIG] for k in ("fwd", "dgrad")]
    assert any(R.has_tie(r) for r in conv)
    assert any(R.has_tie(r) for r in gemm)


TIER_B = [(1, "bf16"), (0, "f32"), (2, "s16"), (2, "one")]


@pytest.mark.parametrize("prec,fam", TIER_B)
@pytest.mark.parametrize("side,label,build", ALL, ids=IDS)
def test_bounded_tier_sees_one_dropped_product(side, label, build, prec, fam):
    """In every contraction the bounded tier checks (tier_b_ok), leaving out ONE product of median size moves the result out of the
    bound in at least half of the output elements -- with the lo*lo allowance and with the bf16 store's half ulp where they apply.
    Evaluated on the operands as drawn: the power-of-two scaling of a non-contracted axis multiplies the products, S, the
    reference and so the bound of an output by one and the same factor."""
    checked = 0
    for name, e in build(fam, scale=False).items():
        if name == "dgrad_sum" or not R.tier_b_ok(e["terms"], prec):
            continue
        a, b = [v.double().flatten() for k, v in e.items() if k not in ("ref", "S", "terms")]
        gen = torch.Generator().manual_seed(0)
        m = (a[torch.randint(0, a.numel(), (100000,), generator=gen)] * b[torch.randint(0, b.numel(), (100000,), generator=gen)]).abs().median()
        # (fp32 form of the output, and its bf16-stored form where a kernel of the bf16 mode stores one: feature maps, gemm_bf16's Cb)
        for stored in (False, True) if prec == 1 and name in stored_outputs(side, label) else (False,):
            bnd = R.bound_of(e["ref"], e["S"], e["terms"] * (4 if prec == 2 else 1), stored, lolo=prec == 2)
            frac = float((m > bnd).double().mean())
            assert frac >= 0.5, (label, name, prec, fam, stored, frac)
        checked += 1
    assert checked or all(not R.tier_b_ok(e["terms"], prec) for e in build(fam, scale=False).values())
