"""Inputs, float64 references and elementwise checkers of the exact-arithmetic parity tests (test_exact_cpu.py proves that the
checkers reject wrong results, test_exact_ops_gpu.py applies them to the conv, transposed-conv and GEMM kernels).

Two tiers:
  A  integer operands.  Small integers are bf16 numbers, every product is exact in every precision mode, and fp32 accumulation of
     integers is exact in any order while every partial sum stays below 2^24 -- so a contraction kernel must return the float64
     result exactly (assert_exact), and a bf16-stored output must be its round-to-nearest-even bf16.
  B  fractional operands.  |out - ref| <= (terms + 64) 2^-23 S elementwise (assert_within), S = sum |a||b| of that output: the
     classical bound of `terms` fp32 additions; operands are chosen so that the products themselves are exact (bf16-rounded in bf16
     mode, 16 significant bits in bf16x3 mode, where the (hi, lo) split is exact).
Everything here is CPU code on float64 / integer bit patterns."""
import torch
import torch.nn.functional as F

U23 = 2.0 ** -23          # unit roundoff allowed per fp32 addition (twice the IEEE 2^-24: room for a non-IEEE adder in the bf16 MFMA)
EXTRA_ADDS = 64           # split-K slabs and row-reduction adds on top of the products of one output
LOLO = 2.0 ** -16         # |lo_a||lo_b| <= 2^-16 |a||b|: what the three-product bf16x3 form leaves out
HALF_ULP_BF16 = 2.0 ** -8  # round-to-nearest half ulp of a bf16 store, relative (a truncating store reaches 2^-7)
INT_S_CAP = 2 ** 20       # tier A: S.max() below this (2^24 with margin for accumulate / residual epilogues)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------ inputs
def ints(shape, lo, hi, seed):
    """integer-valued fp32 tensor, uniform over [lo, hi]"""
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed)).float()


def pow2_rows(t, emin, emax, seed, axis=0):
    """t with every slice along `axis` (a NON-contracted axis of the operation) scaled by 2^e, e uniform over [emin, emax]:
    exact, and every product / sum of an output scales with it"""
    e = torch.randint(emin, emax + 1, (t.shape[axis],), generator=_gen(seed)).double()
    shape = [1] * t.dim()
    shape[axis] = -1
    return (t.double() * torch.pow(torch.tensor(2.0, dtype=torch.float64), e).view(shape)).float()


def _bits(t):
    return t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def _from_bits(b):
    b = torch.where(b >= 2 ** 31, b - 2 ** 32, b)
    return b.to(torch.int32).view(torch.float32)


def sig16(t):
    """fp32 rounded (nearest, ties to even) to 16 significant bits -- 15 stored mantissa bits -- on the bit pattern"""
    b = _bits(t.float())
    b = (b + 0x7F + ((b >> 8) & 1)) & 0xFFFFFF00
    return _from_bits(b)


def one_sided(t):
    """positive 16-significant-bit numbers whose bits below the bf16 mantissa are 0111 1111: the lo half of the bf16x3 split is
    positive and 127/256 of a bf16 ulp under BOTH hi rules (rounded hi == truncated hi), so a dropped hi*lo term adds up coherently
    over K instead of averaging out"""
    t = torch.where(t == 0, torch.ones_like(t), t).abs().float()
    return _from_bits((_bits(t) & 0xFFFF0000) | 0x7F00)


def bf16_bits_rne(t32):
    """upper 16 bits of the nearest bf16 (ties to even) of finite fp32 values, by integer arithmetic"""
    b = _bits(t32)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF


def bf16_rne(t64):
    """nearest bf16, ties to even, as a float32 tensor; integer arithmetic on the fp32 bits, no Tensor.bfloat16().  Exact for
    references that are fp32 numbers (tier A); a float64 reference is first rounded to fp32."""
    return _from_bits(bf16_bits_rne(t64.float()) << 16)


def bf16_trunc(t64):
    """the WRONG store: bf16 by dropping the low 16 bits"""
    return _from_bits(_bits(t64.float()) & 0xFFFF0000)


def split_hi_lo(t, truncate):
    """(hi, lo) of the bf16x3 operand split as float64: hi = bf16(a) rounded or truncated, lo = bf16(a - hi)"""
    hi = (bf16_trunc(t) if truncate else bf16_rne(t)).double()
    lo = bf16_rne(t.double() - hi).double()
    return hi, lo


def has_tie(ref64):
    """some reference value lies exactly half way between two bf16 numbers"""
    b = _bits(ref64.float())
    return bool(((b & 0xFFFF) == 0x8000).any()) and bool((ref64.float().double() == ref64).all())


# -------------------------------------------------------------------------------------------------------------- references
def with_S(fn, *ops):
    """(fn on float64 operands, fn on their absolute values): the reference and its abs-companion S = sum |a||b| per output"""
    d = [o.double() for o in ops]
    return fn(*d), fn(*[o.abs() for o in d])


def _grads(fwd, wrt, dy, *ops):
    ops = [o.clone().requires_grad_(i in wrt) for i, o in enumerate(ops)]
    out = fwd(*ops)
    return torch.autograd.grad(out, [ops[i] for i in wrt], dy)


def conv_fwd(x, w, pad=None):
    """x [B,C,D,H,W], w [Co,Ci,k,k,k], 'same' padding"""
    return F.conv3d(x, w, padding=w.shape[-1] // 2 if pad is None else pad)


def conv_dgrad(dy, w):
    x0 = torch.zeros(dy.shape[0], w.shape[1], *dy.shape[2:], dtype=dy.dtype)
    return _grads(conv_fwd, (0,), dy, x0, w)[0]


def conv_wgrad(x, dy, ks):
    w0 = torch.zeros(dy.shape[1], x.shape[1], ks, ks, ks, dtype=x.dtype)
    return _grads(conv_fwd, (1,), dy, x, w0)[0]


def tconv_fwd(x, w):
    """x [B,Ci,D,H,W], w [Ci,Co,2,2,2], stride 2"""
    return F.conv_transpose3d(x, w, stride=2)


def tconv_dgrad(dy, w):
    x0 = torch.zeros(dy.shape[0], w.shape[0], *[s // 2 for s in dy.shape[2:]], dtype=dy.dtype)
    return _grads(tconv_fwd, (0,), dy, x0, w)[0]


def tconv_wgrad(x, dy):
    w0 = torch.zeros(x.shape[1], dy.shape[1], 2, 2, 2, dtype=x.dtype)
    return _grads(tconv_fwd, (1,), dy, x, w0)[0]


def cl(x):
    """NCDHW -> channels-last"""
    return x.permute(0, 2, 3, 4, 1).contiguous()


# ---------------------------------------------------------------------------------------------------------------- checkers
def _fail(what, bad, out, ref, extra=""):
    n = int(bad.sum())
    err = torch.where(bad, (out - ref).abs(), torch.zeros_like(ref))
    i = int(err.flatten().argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape)) if ref.dim() else ()
    raise AssertionError(f"{what}: {n} of {ref.numel()} elements off; worst at {idx}: got {out.flatten()[i].item()!r}, "
                         f"reference {ref.flatten()[i].item()!r}{extra}")


def _prep(out, ref64, stored_bf16):
    out = out.detach().cpu()
    assert out.dtype == (torch.bfloat16 if stored_bf16 else torch.float32), f"output stored as {out.dtype}"
    assert tuple(out.shape) == tuple(ref64.shape), f"shape {tuple(out.shape)} vs reference {tuple(ref64.shape)}"
    return out.double(), ref64.double()


def assert_exact(out, ref64, stored_bf16, what="output"):
    """out == ref64 in every bit (the sign of a zero aside), or == bf16_rne(ref64) for a bf16-stored output"""
    out, ref = _prep(out, ref64, stored_bf16)
    assert bool((ref.float().double() == ref).all()), f"{what}: the reference itself is not exact in fp32"
    want = bf16_rne(ref).double() if stored_bf16 else ref
    bad = ~(out == want)                    # (NaN compares unequal and is counted)
    if bool(bad.any()):
        _fail(what, bad, out, want)


def bound_of(ref64, S, terms, stored_bf16, lolo):
    E = (terms + EXTRA_ADDS) * U23 * S + (LOLO * S if lolo else 0.0)
    return E + HALF_ULP_BF16 * (ref64.abs() + E) if stored_bf16 else E


def assert_within(out, ref64, S, terms, stored_bf16, lolo=False, what="output"):
    """|out - ref| <= E (+ 2^-8 (|ref| + E) for a bf16 store) elementwise, E = (terms + 64) 2^-23 S (+ 2^-16 S with lolo).
    Returns the largest |out - ref| / bound (a figure to record, never to assert on)."""
    out, ref = _prep(out, ref64, stored_bf16)
    bnd = bound_of(ref, S.double(), terms, stored_bf16, lolo)
    err = (out - ref).abs()
    bad = ~(err <= bnd)
    if bool(bad.any()):
        i = int(torch.where(bad, err / bnd.clamp_min(1e-300), torch.zeros_like(err)).flatten().argmax())
        _fail(what, bad, out, ref, f" (worst ratio |err| / bound = {(err.flatten()[i] / bnd.flatten()[i].clamp_min(1e-300)).item():.3g})")
    nz = bnd > 0
    return float((err[nz] / bnd[nz]).max()) if bool(nz.any()) else 0.0


# ------------------------------------------------------------------------------------- operand families and per-case references
TIER_B_FAMILIES = {0: ("f32",), 1: ("bf16",), 2: ("s16", "one")}   # prec -> families whose products the kernels form exactly
INT_RANGE = {"act": 4, "w": 3, "dy": 4}


def operand(fam, kind, shape, seed, rng=None):
    """one operand of family `fam`: "int" (tier A; |v| <= rng or 4 / 3 / 4 for activations / weights / dy), "f32" (unrounded
    randn), "bf16" (randn pre-rounded to bf16: the kernel's own operand rounding changes nothing), "s16" (16 significant bits: the
    bf16x3 split is exact), "one" (one_sided)."""
    if fam == "int":
        r = INT_RANGE[kind] if rng is None else rng
        return ints(shape, -r, r, seed)
    t = torch.randn(tuple(shape), generator=_gen(seed))
    if fam == "f32":
        return t
    if fam == "bf16":
        return bf16_rne(t)
    if fam == "s16":
        return sig16(t)
    assert fam == "one"
    return one_sided(t)


INT_SCALE = 3             # tier A: 2^-3 .. 2^3 per channel / row


def _scaled(t, fam, seed, axis, scale=True):
    """channels / rows of a non-contracted axis scaled by powers of two: 2^-6 .. 2^6 in tier B, 2^-3 .. 2^3 on the integers of
    tier A (still bf16 numbers; every product and partial sum of an output carries the same factor, so exactness is kept and the
    bf16 stores and their ties land in many binades).  scale=False of the builders: left as drawn."""
    if not scale:
        return t
    r = INT_SCALE if fam == "int" else 6
    return pow2_rows(t, -r, r, seed, axis)


def _entry(fn, terms, **ops):
    ref, S = with_S(fn, *ops.values())
    return dict(ops, ref=ref, S=S, terms=terms)


_cache = {}


def _cached(key, build):
    """references are computed once and shared by the tests that need them"""
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def conv_ops(case, fam, ks=3, rng=None, scale=True):
    """the three contractions of a ks^3 'same' conv (and of the 1x1x1 conv on the same input, the residual branch) on case
    (B, (D, H, W), cin, cout).  NCDHW float32 operands; each entry carries ref / S (float64) and the products per output."""
    def build():
        B, (D, H, W), cin, cout = case
        op = lambda kind, shape, seed: operand(fam, kind, shape, seed, rng)
        sc = lambda t, seed, axis: _scaled(t, fam, seed, axis, scale)
        xs, ys = (B, cin, D, H, W), (B, cout, D, H, W)
        w, w3 = op("w", (cout, cin, ks, ks, ks), 2), op("w", (cout, cin, 1, 1, 1), 5)
        r = {}
        x = sc(op("act", xs, 1), 11, 0)
        r["fwd"] = _entry(conv_fwd, cin * ks ** 3, x=x, w=sc(w, 12, 0))
        r["fwd3"] = _entry(conv_fwd, cin, x=x, w=sc(w3, 13, 0))
        dy, dy3 = sc(op("dy", ys, 3), 14, 0), sc(op("dy", ys, 6), 14, 0)
        wd, w3d = sc(w, 15, 1), sc(w3, 15, 1)
        r["dgrad"] = _entry(conv_dgrad, cout * ks ** 3, dy=dy, w=wd)
        r["dgrad3"] = _entry(conv_dgrad, cout, dy=dy3, w=w3d)
        r["dgrad_sum"] = dict(ref=r["dgrad"]["ref"] + r["dgrad3"]["ref"], S=r["dgrad"]["S"] + r["dgrad3"]["S"], terms=cout * (ks ** 3 + 1))
        xw = sc(op("act", xs, 7), 16, 1)
        r["wgrad"] = _entry(lambda a, b: conv_wgrad(a, b, ks), B * D * H * W, x=xw, dy=sc(op("dy", ys, 8), 17, 1))
        r["wgrad3"] = _entry(lambda a, b: conv_wgrad(a, b, 1), B * D * H * W, x=xw, dy=sc(op("dy", ys, 9), 18, 1))
        return r
    return _cached(("conv", case, fam, ks, rng, scale), build)


def tconv_ops(case, fam, rng=None, scale=True):
    """the three contractions of the 2x2x2 stride-2 transposed conv on case (B, S, cin, cout)"""
    def build():
        B, S, cin, cout = case
        op = lambda kind, shape, seed: operand(fam, kind, shape, seed, rng)
        sc = lambda t, seed, axis: _scaled(t, fam, seed, axis, scale)
        xs, ys = (B, cin, S, S, S), (B, cout, 2 * S, 2 * S, 2 * S)
        w = op("w", (cin, cout, 2, 2, 2), 2)
        r = {}
        r["fwd"] = _entry(tconv_fwd, cin, x=sc(op("act", xs, 1), 11, 0), w=sc(w, 12, 1))
        r["dgrad"] = _entry(tconv_dgrad, 8 * cout, dy=sc(op("dy", ys, 3), 14, 0), w=sc(w, 15, 0))
        r["wgrad"] = _entry(tconv_wgrad, B * S ** 3, x=sc(op("act", xs, 7), 16, 1), dy=sc(op("dy", ys, 8), 17, 1))
        return r
    return _cached(("tconv", case, fam, rng, scale), build)


def gemm_ops(case, fam, rng=None, scale=True):
    """y = x w^T, dx = dy w, dw = dy^T x on case (M, N, K): x [M,K], w [N,K], dy [M,N]"""
    def build():
        M, N, K = case
        op = lambda kind, shape, seed: operand(fam, kind, shape, seed, rng)
        sc = lambda t, seed, axis: _scaled(t, fam, seed, axis, scale)
        w = op("w", (N, K), 2)
        r = {}
        r["fwd"] = _entry(lambda a, b: a @ b.t(), K, x=sc(op("act", (M, K), 1), 11, 0), w=sc(w, 12, 0))
        r["dgrad"] = _entry(lambda a, b: a @ b, N, dy=sc(op("dy", (M, N), 3), 14, 0), w=sc(w, 15, 1))
        r["wgrad"] = _entry(lambda a, b: a.t() @ b, M, dy=sc(op("dy", (M, N), 8), 17, 1), x=sc(op("act", (M, K), 7), 16, 1))
        return r
    return _cached(("gemm", case, fam, rng, scale), build)


def tier_b_ok(K, prec):
    """Contraction lengths the bounded tier takes.  A dropped product has to stand out of the allowance E = terms 2^-23 S with
    S ~ K mean|ab| and terms = K (4 K in bf16x3 mode); the median of |ab| for independent normal a, b is ~0.49 of its mean, so
    terms K 2^-23 has to stay below that with margin: K <= 1728 (K <= 864 in bf16x3 mode)."""
    return (4 if prec == 2 else 1) * K * K * U23 <= 0.36
