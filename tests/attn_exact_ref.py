"""Inputs, references, checkers and a chunked float64 emulation for the exact-arithmetic parity tests of the attention kernels
(csrc/attention.hip, csrc/attention_b16.hip).  tests/test_attn_exact_cpu.py proves on the CPU that the inputs are what they claim
to be and that the checkers reject wrong kernels; tests/test_attn_exact_gpu.py applies the same checkers to the kernels.

Inputs.  The head dim is split into three bands.  Group band (16 dims): key j carries a single 1 at the dim of its group, query i
carries -2048 on every group it does not allow and 0 on the ones it allows, so q.k is exactly 0 (allowed) or -2048 (scaled: -362,
-256, -181 for head dim 32, 64, 128; fp32 exp is 0 below -104).  "k free" band: k holds data, q zeros (feeds dq).  "q free" band:
q holds data, k zeros (feeds dk).  The keys at the edges of the kernel under test (tile = 32 keys for the generic kernels, 224 for
the bf16-storage kernels) get singleton groups, the others three bulk groups; every (batch item, head) has its own data, its own
assignment of groups to dims and its own rotation of the query plans.

Families: "int" (small integers everywhere: the softmax and everything after it is exact where the set size is a power of two),
"frac" (the same score structure, data from the fractional generators of exact_ref.py, set sizes 3 / 5 / 6 / 25 too) and "mod"
("frac" plus four dims in which BOTH q and k hold multiples of 1/4: exact scores of magnitude up to SMAX after scaling, so that
exp is the only inexact operation in P).

Tier A: exact.  Tier B: |out - ref| <= allowance * (sum of absolute terms of that element) -- see allowances()."""
import math

import torch

import exact_ref as R
from exact_ref import EXTRA_ADDS, HALF_ULP_BF16, LOLO, U23

G = 16                    # dims of the group band
NEG = -2048.0             # q entry on a disallowed group
SMAX = 16.0               # "mod" family: |score * scale| <= SMAX, so |lse| < 32 and exp arguments are >= -2 SMAX
#                           (16 rather than 30: the half ulp of an fp32 lse below 32 is 2^-20, which 8 x still keeps under the 2^-17 cap of
#                           EXPLOG; at 32 <= lse < 64 the rounding of lse alone would exceed it and say nothing about exp or log)
# Relative error of one exp / log evaluation of the kernels (expf / logf in attention.hip, __expf / __logf in attention_b16.hip).
# Not derivable from the project: measured on an MI355X as the largest |lse - lse_ref| over the one-hot / power-of-two rows of the
# "int" family and all rows of the "mod" family in fp32 mode against the float64 reference (test_explog_measure; the figure is in
# profiles/exact_parity.txt), then multiplied by 8 -- the other shapes, and exp(s - lse) in the backward, which stacks two
# evaluations -- and capped at 2^-17 so that it stays under the 2^-16 hi*lo term of the bf16x3 mode.  Measured: 5.714e-09 on the
# integer rows, 8.781e-07 on the moderate-score rows (which is mostly the half ulp, 2^-20 = 9.5e-07, of an lse between 16 and 32
# itself: the figure bounds the evaluation error from above); 8 x 8.79e-07 = 7.03e-06 < 2^-17 = 7.63e-06, so the cap does not bind.
EXPLOG_MEASURED = 8.79e-07
EXPLOG = min(8 * EXPLOG_MEASURED, 2.0 ** -17)

# mode -> what the kernels of that mode do to the intermediates.  T: keys per tile / chunk of the online softmax; fam: the
# fractional generator whose products the mode forms exactly; round: P (for dv and out) and dS are rounded to bf16 before their
# MFMA; lolo: they are split (hi, lo) instead; stored: delta is formed from the bf16-STORED output.
MODES = {
    "f32": dict(prec=0, T=32, fam="f32", round=False, lolo=False, stored=False),
    "bf16": dict(prec=1, T=32, fam="bf16", round=True, lolo=False, stored=False),
    "x3": dict(prec=2, T=32, fam="s16", round=False, lolo=True, stored=False),
    "b16": dict(prec=1, T=224, fam="bf16", round=True, lolo=False, stored=True),
}
GENERIC_MODES = ("f32", "bf16", "x3")
KINDS = ("int", "frac", "mod")


def scale32(dh):
    """the scale the entry points pass, as the fp32 number the kernels receive"""
    return float(torch.tensor(float(dh) ** -0.5, dtype=torch.float32))


# -------------------------------------------------------------------------------------------------------------- construction
def key_groups(L, T):
    """(groups, win, singles): groups = list of key lists -- singletons for the edge keys, then the bulk groups A (25 keys spread over the
    whole range: 1/25 is a number whose TRUNCATION to bf16 is off by 1.31 half ulps), lower and upper; win = the eight keys around
    the boundary bd (end of the first tile / chunk; a 16-boundary or the middle where L has no such boundary), nearest first; singles = the edge keys."""
    bd = T if L > T else (16 if L > 16 else max(L // 2, 1))
    win = sorted(range(max(0, bd - 8), min(L, bd + 8)), key=lambda j: (abs(j - (bd - 0.5)), j))[:8]
    tl = ((L - 1) // T) * T                   # first key of the last tile / chunk
    e16 = ((L - 1) // 16) * 16 - 1            # last key before the last 16-boundary
    singles = sorted(set(win) | {j for j in (0, L - 1, tl - 1, tl, e16) if 0 <= j < L})
    rest = [j for j in range(L) if j not in set(singles)]
    A = rest[::max(1, len(rest) // 25)][:25] if len(rest) >= 50 else rest[:len(rest) // 3]
    lower = [j for j in rest if j not in set(A) and j < L // 2]
    upper = [j for j in rest if j not in set(A) and j >= L // 2]
    groups = [[j] for j in singles] + [g for g in (A, lower, upper) if g]
    assert len(groups) <= G
    return groups, win, singles


def plans(L, T, kind):
    """list of (name, allowed keys).  One-hot rows on every edge key (those on keys of a later tile are "max rises" rows: the whole
    first tile scores -2048; those on keys of the first tile are "max falls" rows), sets of 2 / 4 / 8 straddling the boundary, the
    bulk sets; the fractional families add 3 / 5 / 6 keys around the boundary and the row that allows every key."""
    groups, win, singles = key_groups(L, T)
    out = [("onehot%d" % j, [j]) for j in singles]
    sizes = (2, 4, 8) if kind == "int" else (2, 3, 4, 5, 6, 8)
    out += [("set%d" % n, sorted(win[:n])) for n in sizes if n <= len(win)]
    out += [("bulk%d" % i, g) for i, g in enumerate(groups[len(singles):])]
    if kind != "int":
        out.append(("all", list(range(L))))
    return out


class Case:
    """one attention problem: inputs in the kernels' layout, the float64 reference, its abs-companions and the tier-A masks"""

    def __init__(self, dh, L, B, heads, T, kind, fam):
        self.dh, self.L, self.B, self.heads, self.T, self.kind, self.fam = dh, L, B, heads, T, kind, fam
        self.scale = scale32(dh)
        self.name = f"dh{dh}-L{L}-B{B}-h{heads}-T{T}-{kind}-{fam}"
        self._build()
        self._reference()

    # ---- inputs
    def _data(self, shape, lo, hi, seed):
        if self.kind == "int":
            return R.ints(shape, lo, hi, seed).double()
        return R.operand(self.fam, "act", shape, seed).double()

    def _build(self):
        dh, L, T, BH = self.dh, self.L, self.T, self.B * self.heads
        F = (dh - G) // 2
        groups, win, singles = key_groups(L, T)
        pl = plans(L, T, self.kind)
        gid = torch.empty(L, dtype=torch.long)
        for g, keys in enumerate(groups):
            gid[keys] = g
        q, k = torch.zeros(BH, L, dh, dtype=torch.float64), torch.zeros(BH, L, dh, dtype=torch.float64)
        self.plan_of = torch.empty(BH, L, dtype=torch.long)
        rows = torch.arange(L)
        for bh in range(BH):
            perm = torch.randperm(G, generator=R._gen(1000 + bh))          # group -> dim, different per (b, h)
            k[bh, rows, perm[gid]] = 1.0
            p_of = (rows + 5 * (rows // 16) + 3 * bh) % len(pl)             # every 16-row tile sees a different run of plans
            self.plan_of[bh] = p_of
            allow = torch.zeros(len(pl), G, dtype=torch.bool)
            for p, (_, keys) in enumerate(pl):
                allow[p, gid[keys]] = True
            qg = torch.full((L, G), NEG, dtype=torch.float64)
            rr, gg = allow[p_of].nonzero(as_tuple=True)
            qg[rr, perm[gg]] = 0.0
            q[bh, :, :G] = qg
        k[:, :, G:G + F] = self._data((BH, L, F), -3, 3, 2)
        q[:, :, G + F:] = self._data((BH, L, dh - G - F), -3, 3, 3)
        if self.kind == "mod":                       # four dims that both q and k fill: multiples of 1/4, 4 r^2 scale <= SMAX
            r4 = int(4 * math.sqrt(SMAX / (4 * self.scale)))
            q[:, :, G:G + 4] = R.ints((BH, L, 4), -r4, r4, 4).double() / 4
            k[:, :, G:G + 4] = R.ints((BH, L, 4), -r4, r4, 5).double() / 4
        v = self._data((BH, L, dh), -4, 4, 6)
        nz = torch.rand(BH, L, dh, generator=R._gen(7)).argsort(-1) < 3          # three non-zeros per row of dout
        do = torch.where(nz, self._data((BH, L, dh), -2, 2, 8), torch.zeros((), dtype=torch.float64))
        self.q, self.k, self.v, self.do, self.plans_ = q, k, v, do, pl
        for t in (q, k, v, do):                       # every operand is a number of the mode's format
            assert bool((t.float().double() == t).all())
            if self.fam in ("int", "bf16"):
                assert bool((R.bf16_rne(t).double() == t).all())
            elif self.fam == "s16":
                assert bool((R.sig16(t.float()).double() == t).all())
        self.qkv = self.pack3(q, k, v).float()
        self.dout = self.pack1(do).float()

    # ---- layouts: [BH, L, dh] <-> [B*L, heads*dh] / [B*L, 3*heads*dh]
    def pack1(self, t):
        return t.reshape(self.B, self.heads, self.L, -1).permute(0, 2, 1, 3).reshape(self.B * self.L, -1).contiguous()

    def pack3(self, a, b, c):
        t = torch.stack([a, b, c]).view(3, self.B, self.heads, self.L, self.dh)
        return t.permute(1, 3, 0, 2, 4).reshape(self.B * self.L, 3 * self.heads * self.dh).contiguous()

    def rowmask1(self, rows):
        """[BH, L] bool -> mask in the layout of out"""
        return self.pack1(rows[:, :, None].expand(-1, -1, self.dh))

    def where(self, row, col, three):
        """(batch item, token, which of q/k/v, head, dim, tile of the token) of an element of out / dqkv"""
        Hd = self.heads * self.dh
        which, c = (col // Hd, col % Hd) if three else (0, col)
        return (f"batch {row // self.L} token {row % self.L} ({'qkv'[which] if three else 'out'}) head {c // self.dh} dim {c % self.dh}; "
                f"token is row {row % self.L % self.T} of {self.T}-tile {row % self.L // self.T}, 16-row tile {row % self.L // 16}")

    # ---- reference
    def _reference(self):
        q, k, v, do, sc_ = self.q, self.k, self.v, self.do, self.scale
        s = (q @ k.transpose(1, 2)) * sc_                                   # exact: one non-zero product of the group band (+ 4)
        M = s > -100.0
        self.M, self.s = M, s
        mx = torch.where(M, s, torch.full_like(s, -1e300)).amax(-1, keepdim=True)
        e = torch.where(M, torch.exp(s - mx), torch.zeros_like(s))           # disallowed pairs: exactly 0, no 1e-112 residue
        l = e.sum(-1, keepdim=True)
        P = e / l                                                            # set families: M / |S_i|, exact for |S_i| = 2^n
        self.P, self.n = P, M.sum(-1)
        self.lse = (mx + torch.log(l)).squeeze(-1)                           # 0 + log |S_i|
        out, S_out = P @ v, P @ v.abs()
        dP, SdP = do @ v.transpose(1, 2), do.abs() @ v.abs().transpose(1, 2)
        delta, Sdelta = (P * dP).sum(-1, keepdim=True), (P * SdP).sum(-1, keepdim=True)
        dS, Tm = P * (dP - delta), P * (SdP + Sdelta)
        self.dP, self.delta, self.dS = dP, delta, dS
        self.raw = dict(dq=dS @ k, dk=dS.transpose(1, 2) @ q, Sdq=dS.abs() @ k.abs(), Sdk=dS.abs().transpose(1, 2) @ q.abs())
        dq, dk, dv = sc_ * (dS @ k), sc_ * (dS.transpose(1, 2) @ q), P.transpose(1, 2) @ do
        Sdq, Sdk, Sdv = sc_ * (Tm @ k.abs()), sc_ * (Tm.transpose(1, 2) @ q.abs()), P.transpose(1, 2) @ do.abs()
        self.out_bh, self.S_out_bh = out, S_out
        self.out, self.S_out = self.pack1(out), self.pack1(S_out)
        self.dqkv, self.S_dqkv = self.pack3(dq, dk, dv), self.pack3(Sdq, Sdk, Sdv)

    # ---- tier A: which rows / keys are exact in a mode.  Decided HERE, by bit checks on the reference; never by a GPU result
    def tier_a(self, mode):
        """dict of [BH, L] bool masks: lse (one-hot rows), fwd (rows whose out is exact), dq (rows whose dq is exact), dkv (keys whose
        dk and dv are exact), plus "why": what moved rows out of tier A"""
        md = MODES[mode]
        none = torch.zeros(self.B * self.heads, self.L, dtype=torch.bool)
        if self.kind != "int":
            return dict(lse=none, fwd=none, dq=none, dkv=none, why="fractional data: accumulation rounds")
        n = self.n
        onehot, pow2 = n == 1, (n == 2) | (n == 4) | (n == 8)
        fp32 = lambda t: (t.float().double() == t)
        b16 = lambda t: (R.bf16_rne(t).double() == t)
        fwd = (onehot | pow2) & fp32(self.P).all(-1) & fp32(self.out_bh).all(-1)
        bwd = onehot.clone()
        why = "power-of-two rows: exp(-logf(2^n)) is not 2^-n in fp32 and the mode does not round P"
        if md["round"]:       # P rounds to 2^-n; dS = p (dP - delta) rounds to its exact value iff that value is a bf16 number
            ok = pow2 & fp32(self.delta).all(-1) & b16(self.dS).all(-1) & b16(self.P).all(-1)
            if md["stored"]:  # delta is formed from the bf16-stored out: it must be that out
                ok &= b16(self.out_bh).all(-1)
            bwd |= ok
            why = "power-of-two rows whose dS = (dP - delta) / |S| needs more than 8 significant bits"
        Mb = self.M
        dkv = ~(Mb & ~bwd[:, :, None]).any(1)            # every row that allows the key is an exact row
        return dict(lse=onehot, fwd=fwd, dq=bwd, dkv=dkv, why=why)


_cases = {}


def case(dh, L, B, heads, mode, kind):
    """cached: the reference is computed once and shared by the tests that need it"""
    T = MODES[mode]["T"]
    fam = "int" if kind == "int" else MODES[mode]["fam"]
    key = (dh, L, B, heads, T, kind, fam)
    if key not in _cases:
        _cases[key] = Case(*key)
    return _cases[key]


# ------------------------------------------------------------------------------------------------------------------ tier B
def allowances(c, mode):
    """Relative allowances of tier B, each multiplying the element's sum of absolute terms (S_out = sum_j p |v|;
    S_dv = sum_i p |dout|; S_dq = scale sum_j p (sum_d |dout||v| + sum_d |dout| S_out) |k|, S_dk alike with |q|).

      acc(n) = (n [x 4 in bf16x3 mode: four products per element] + EXTRA_ADDS) U23      n fp32 additions, tile rescales included
      e_p    = EXPLOG + 2 SMAX U23       one exp of an argument of magnitude <= 2 SMAX: the evaluation, and the rounding of the
                                         argument (s * scale, s - m, the fast exp's x * log2 e), which exp turns into a relative error
      r_p    = HALF_ULP_BF16 | LOLO | 0  P and dS as MFMA operands: rounded to bf16 / split into (hi, lo) / fp32
      out:   l and o each carry acc(L) and e_p; P entering o carries r_p; 1 / l and the product are 2 roundings (3 U23 with the store)
      lse:   absolute.  l carries acc(L) + e_p relative, log turns that into an absolute error; logf itself EXPLOG |log l|
             <= EXPLOG (|lse| + SMAX); the sum m + log l one rounding of |lse|
      p_bwd: exp(s - lse): e_p, plus the absolute error of lse
      dS = p (dP - delta): p_bwd; dP acc(dh); delta acc(dh) and the error of out (plus HALF_ULP_BF16 where delta is formed from
             the bf16-STORED out); the subtraction and the product 3 U23; r_p for dS as an operand
      dq, dk: dS, acc(L), the multiplication by scale;   dv: p_bwd, r_p, acc(L)"""
    md = MODES[mode]
    acc = lambda n: (n * (4 if md["lolo"] else 1) + EXTRA_ADDS) * U23
    e_p = EXPLOG + 2 * SMAX * U23
    r_p = HALF_ULP_BF16 if md["round"] else (LOLO if md["lolo"] else 0.0)
    lmax = float(c.lse.abs().max())
    a_out = 2 * acc(c.L) + 2 * e_p + r_p + 3 * U23
    a_lse = acc(c.L) + e_p + EXPLOG * (lmax + SMAX) + 2 * U23 * (1 + lmax)
    p_bwd = e_p + a_lse
    a_dS = p_bwd + 2 * acc(c.dh) + a_out + (HALF_ULP_BF16 if md["stored"] else 0.0) + 3 * U23 + r_p
    return dict(out=a_out, lse=a_lse, dq=a_dS + acc(c.L) + 2 * U23, dv=p_bwd + r_p + acc(c.L) + U23)


def assert_bounded(out, ref64, E, stored_bf16, what, loc=None):
    """|out - ref| <= E (+ 2^-8 (|ref| + E) for a bf16 store) elementwise, in the style of exact_ref.assert_within; returns the
    largest |out - ref| / bound"""
    out, ref = R._prep(out, ref64, stored_bf16)
    bnd = E + HALF_ULP_BF16 * (ref.abs() + E) if stored_bf16 else E
    err = (out - ref).abs()
    bad = ~(err <= bnd)
    if bool(bad.any()):
        i = int(torch.where(bad, err / bnd.clamp_min(1e-300), torch.zeros_like(err)).flatten().argmax())
        at = "" if loc is None else " -- " + loc(i)
        R._fail(what, bad, out, ref, f" (worst ratio |err| / bound = {(err.flatten()[i] / bnd.flatten()[i].clamp_min(1e-300)).item():.3g}){at}")
    nz = bnd > 0
    return float((err[nz] / bnd[nz]).max()) if bool(nz.any()) else 0.0


def _exact_on(mask, out, ref64, stored, what, loc):
    """exact_ref.assert_exact on the elements of `mask` (the others are replaced by what is expected of them)"""
    if not bool(mask.any()):
        return
    out = out.detach().cpu()
    ref = ref64.float().double()                  # tier A: the one rounding of dq * scale / dk * scale for head dims 32, 128
    want = R.bf16_rne(ref).bfloat16() if stored else ref.float()
    try:
        R.assert_exact(torch.where(mask, out, want), ref, stored, what)
    except AssertionError as e:
        bad = mask & ~(out.double() == want.double())
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{e} -- first at {loc(i)}") from None


def check(c, mode, res, ratios=None, label="", tiers="AB", exact=None):
    """Both tiers on whatever of out / out_b / lse / dqkv / dqkv_b `res` holds (float32 tensors, *_b bfloat16).  Tier A on the
    rows / keys c.tier_a(mode) names, tier B on every element (tiers: which of the two run).  Appends (label, case, mode, output, ratio) to `ratios` and
    (label, mode, output, number of elements that were compared bit for bit) to `exact`."""
    ta, al = c.tier_a(mode), allowances(c, mode)
    Hd = c.heads * c.dh
    what = lambda o: f"{label} {c.name} mode {mode} {o}"
    loc1 = lambda i: c.where(i // Hd, i % Hd, False)
    loc3 = lambda i: c.where(i // (3 * Hd), i % (3 * Hd), True)
    lse_ref = c.lse.view(c.B, c.heads, c.L)
    done, tally = [], []
    for key, stored in (("out", False), ("out_b", True)):
        if res.get(key) is not None:
            if "A" in tiers:
                _exact_on(c.rowmask1(ta["fwd"]), res[key], c.out, stored, what(key + " tier A"), loc1)
                tally.append((key, int(ta["fwd"].sum()) * c.dh))
            if "B" in tiers:
                done.append((key, assert_bounded(res[key], c.out, al["out"] * c.S_out, stored, what(key), loc1)))
    if res.get("lse") is not None:
        lse = res["lse"].detach().cpu()
        locl = lambda i: f"batch {i // (c.heads * c.L)} head {i // c.L % c.heads} query {i % c.L} (plan {c.plans_[int(c.plan_of.flatten()[i])][0]})"
        if "A" in tiers:
            _exact_on(ta["lse"].view_as(lse_ref), lse, lse_ref, False, what("lse tier A"), locl)
            tally.append(("lse", int(ta["lse"].sum())))
        if "B" in tiers:
            done.append(("lse", assert_bounded(lse, lse_ref, torch.full_like(lse_ref, al["lse"]), False, what("lse"), locl)))
    m3 = c.pack3(*(m[:, :, None].expand(-1, -1, c.dh) for m in (ta["dq"], ta["dkv"], ta["dkv"])))
    E3 = c.S_dqkv.clone()
    E3[:, :2 * Hd] *= al["dq"]
    E3[:, 2 * Hd:] *= al["dv"]
    for key, stored in (("dqkv", False), ("dqkv_b", True)):
        if res.get(key) is not None:
            if "A" in tiers:
                _exact_on(m3, res[key], c.dqkv, stored, what(key + " tier A"), loc3)
                tally += [(key + ".dq", int(ta["dq"].sum()) * c.dh), (key + ".dk,dv", 2 * int(ta["dkv"].sum()) * c.dh)]
            for i, nm in enumerate("qkv" if "B" in tiers else ""):
                sl = slice(i * Hd, (i + 1) * Hd)
                locp = lambda j, i=i: c.where(j // Hd, i * Hd + j % Hd, True)
                done.append((f"{key}.d{nm}", assert_bounded(res[key][:, sl], c.dqkv[:, sl], E3[:, sl], stored, what(f"{key} d{nm}"), locp)))
    if ratios is not None:
        ratios.extend((label, c.name, mode, o, r) for o, r in done)
    if exact is not None and c.kind == "int":
        exact.extend((label, mode, o, n, n0) for (o, n), n0 in zip(tally, _sizes(c, tally)))
    return done


def _sizes(c, tally):
    """number of elements of each tallied output"""
    n = c.B * c.heads * c.L
    return [n if o == "lse" else (2 if o.endswith("dk,dv") else 1) * n * c.dh for o, _ in tally]


# ------------------------------------------------------------------------------------------- chunked online-softmax emulation
MUTANTS = ("drop_last_key", "pad_key", "l_not_rescaled", "o_not_rescaled", "p_truncated", "no_delta_last_chunk", "clamped_queries",
           "last_query_tile_missing", "dq_scaled_twice", "dk_not_scaled", "neighbour_k")


def emulate(c, mode, chunk=None, mutant=None):
    """float64 emulation of the kernels' algorithm on case c: forward with a running max / sum over chunks of `chunk` keys, the dQ
    role (query on the lane, loop over key chunks) and the dK/dV role (key on the lane, loop over query chunks), with the mode's
    bf16 roundings of P and dS.  `mutant` names one deliberate error.  Returns the outputs check() takes."""
    md = MODES[mode]
    chunk = chunk or md["T"]
    L, sc_ = c.L, c.scale
    q, k, v, do = c.q, c.k, c.v, c.do
    if mutant == "neighbour_k":
        k = k.roll(1, 0)
    rnd = (lambda t: R.bf16_rne(t).double()) if md["round"] else (lambda t: t)
    rnd_p = (lambda t: R.bf16_trunc(t).double()) if mutant == "p_truncated" else rnd
    starts = list(range(0, L, chunk))

    def keys_of(k0):
        idx = list(range(k0, min(k0 + chunk, L)))
        ragged = k0 == starts[-1] and len(idx) % chunk
        if ragged and mutant == "drop_last_key":
            idx = idx[:-1]
        if ragged and mutant == "pad_key":
            idx = idx + [L - 1]
        return idx

    BH = q.shape[0]
    m = torch.full((BH, L, 1), -1e30, dtype=torch.float64)
    l, o = torch.zeros(BH, L, 1, dtype=torch.float64), torch.zeros(BH, L, c.dh, dtype=torch.float64)
    for k0 in starts:
        idx = keys_of(k0)
        if not idx:
            continue
        s = (q @ k[:, idx].transpose(1, 2)) * sc_
        mn = torch.maximum(m, s.amax(-1, keepdim=True))
        alpha, p = torch.exp(m - mn), torch.exp(s - mn)
        l = l * (1.0 if mutant == "l_not_rescaled" else alpha) + p.sum(-1, keepdim=True)
        o = o * (1.0 if mutant == "o_not_rescaled" else alpha) + rnd_p(p) @ v[:, idx]
        m = mn
    out, lse = o / l, m + torch.log(l)
    res = dict(out=c.pack1(out).float(), out_b=c.pack1(R.bf16_rne(out)).bfloat16(), lse=lse.view(c.B, c.heads, L).float())
    delta = (do * (R.bf16_rne(out).double() if md["stored"] else out.float().double())).sum(-1, keepdim=True)
    lse = lse.float().double()
    # dQ role
    dq = torch.zeros_like(o)
    for k0 in starts:
        idx = keys_of(k0)
        if not idx:
            continue
        p = torch.exp((q @ k[:, idx].transpose(1, 2)) * sc_ - lse)
        dp = do @ v[:, idx].transpose(1, 2)
        ds = p * (dp if (mutant == "no_delta_last_chunk" and k0 == starts[-1]) else dp - delta)
        dq += rnd(ds) @ k[:, idx]
    dq *= sc_ * sc_ if mutant == "dq_scaled_twice" else sc_
    # dK/dV role
    dk, dv = torch.zeros_like(o), torch.zeros_like(o)
    for q0 in starts:
        idx = list(range(q0, min(q0 + chunk, L)))
        if q0 == starts[-1]:
            if mutant == "clamped_queries":
                idx += [L - 1] * (-L % 16)
            if mutant == "last_query_tile_missing":
                idx = [i for i in idx if i < (L - 1) // 16 * 16]
        if not idx:
            continue
        p = torch.exp((q[:, idx] @ k.transpose(1, 2)) * sc_ - lse[:, idx])
        dp = do[:, idx] @ v.transpose(1, 2)
        ds = p * (dp if (mutant == "no_delta_last_chunk" and q0 == starts[-1]) else dp - delta[:, idx])
        dv += rnd_p(p).transpose(1, 2) @ do[:, idx]
        dk += rnd(ds).transpose(1, 2) @ q[:, idx]
    if mutant != "dk_not_scaled":
        dk *= sc_
    d3 = c.pack3(dq, dk, dv)
    res.update(dqkv=d3.float(), dqkv_b=R.bf16_rne(d3).bfloat16())
    return res
