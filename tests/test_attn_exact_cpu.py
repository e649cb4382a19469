"""The exact-arithmetic attention tests mean something before a GPU sees them (tests/attn_exact_ref.py):

* representability: by bit checks, for every case and mode, scores are 0 or <= -104 (after the row maximum is taken off, in the
  moderate-score family), every intermediate a mode rounds on a tier-A row is a number of the format it is rounded to, and every
  partial sum is an integer below 2^24 in its unit;
* mutants: a float64 emulation of the chunked online softmax (forward, dQ role, dK/dV role; chunk 32 and 224) passes every case
  unmutated, and each named mutation of it is rejected by the exact tier AND by the bounded tier on at least one case;
* coverage: the case lists of tests/test_attn_exact_gpu.py (defined HERE, imported there) reach the resident and the tiled
  instantiation of all three generic kernels for every precision and head dim, and the full-chunk, ragged and multi-chunk paths of
  the bf16-storage kernels."""
import pytest
import torch

import attn_exact_ref as A
import exact_ref as R

# ---------------------------------------------------------------------------------------------------------------- case lists
GENERIC_L = {64: [33, 216, 290, 530], 32: [33, 530, 1000], 128: [100, 130, 290]}          # head dim -> token counts
B16_L = [8, 216, 224, 225, 230, 449, 1000]
B16_NW4 = (8, 33, 16)          # (L, B, heads): the 4-wave backward of attention_b16.hip (pick_nw: cdiv(L, 32) heads B > 512)


def shape(L):
    """(B, heads)"""
    return (1, 2) if L == 1000 else (2, 2)


GENERIC = [(dh, L) + shape(L) for dh, Ls in GENERIC_L.items() for L in Ls]
B16 = [(64, L) + shape(L) for L in B16_L]
ALL = [(cs, m) for cs in GENERIC for m in A.GENERIC_MODES] + [(cs, "b16") for cs in B16]
ids = lambda p: [f"dh{c[0]}-L{c[1]}-{m}" for c, m in p]


# ------------------------------------------------------------------------------------------------------------ coverage table
def forms(dh, L, mode):
    """(fwd, dq, dkv resident?) as launch_fwd / launch_bwd of csrc/attention.hip decide (lines 398-418, constants of AttnCfg at
    lines 22-30 and ATTN_LDS_MAX at line 390)"""
    ch = 8 if mode == "bf16" else 4                   # P::CH: elements per 16-byte chunk
    img_c = 32 * (dh * (16 // ch) + 16)               # IMG_C = 32 * PC
    nt = -(-L // 32)
    lds_max = 150 * 1024
    return tuple(t * nt <= lds_max for t in (2 * img_c, 2 * img_c, 2 * img_c + 256))


def test_predicates_restate_the_issue_thresholds():
    first_tiled = lambda dh, mode, i: next(L for L in range(1, 4000) if not forms(dh, L, mode)[i])
    assert [first_tiled(32, m, 0) for m in A.GENERIC_MODES] == [513, 961, 513] and first_tiled(32, "bf16", 2) == 897
    assert [first_tiled(128, m, 0) for m in A.GENERIC_MODES] == [129, 257, 129]
    assert forms(32, 930, "bf16") == (True, True, False)        # the three predicates can disagree


def test_coverage_generic():
    for mode in A.GENERIC_MODES:
        for dh in (32, 64, 128):
            seen = [forms(dh, L, mode) for d, L, _, _ in GENERIC if d == dh]
            for i, kern in enumerate(("fwd", "dq", "dkv")):
                assert {f[i] for f in seen} == {True, False}, f"{mode} dh {dh} {kern}: resident and tiled not both reached"


def test_coverage_b16():
    """attention_b16.hip: nkeys = min(224, L - k0), rows = nkeys rounded up to 32, full = rows == 224"""
    paths = set()
    for _, L, _, _ in B16:
        chunks = [min(224, L - k0) for k0 in range(0, L, 224)]
        for n in chunks:
            paths.add("full" if (n + 31) // 32 * 32 == 224 else "ragged")
            if n % 32:
                paths.add("pad keys")
            if n == 224:
                paths.add("exactly full")
        if len(chunks) > 1:
            paths.add("loop")
            if chunks[-1] == 1:
                paths.add("second chunk of one key")
            if (chunks[-1] + 31) // 32 * 32 == 224:
                paths.add("full then full-by-rounding")
    assert paths >= {"full", "ragged", "pad keys", "exactly full", "loop", "second chunk of one key"}
    L, B, heads = B16_NW4
    assert -(-L // 32) * heads * B > 512 and all(-(-L // 32) * h * b <= 512 for _, L, b, h in B16)     # both backward wave counts


def test_edge_keys_are_singletons_and_plans_cover_tiles():
    for (dh, L, B, heads), mode in ALL:
        T = A.MODES[mode]["T"]
        groups, win, singles = A.key_groups(L, T)
        want = {0, L - 1, ((L - 1) // 16) * 16 - 1} | ({T - 1, T} if L > T else set()) | {((L - 1) // T) * T - 1, ((L - 1) // T) * T}
        assert {j for j in want if 0 <= j < L} <= set(singles)
        assert sorted(j for g in groups for j in g) == list(range(L))
        c = A.case(dh, L, B, heads, mode, "int")
        names = [n for n, _ in c.plans_]
        if L > T:             # max rises / max falls rows exist
            assert f"onehot{L - 1}" in names and "onehot0" in names
        for bh in range(B * heads):                       # different (b, h): different plan rotation and different data
            assert not torch.equal(c.q[bh], c.q[(bh + 1) % (B * heads)]) and not torch.equal(c.k[bh], c.k[(bh + 1) % (B * heads)])
        kinds = {n.rstrip("0123456789") for n in names}
        assert kinds >= ({"onehot", "set", "bulk"} if L > 16 else {"onehot", "set"})      # (L = 8: every key is an edge key)
        if L >= 64:                                       # every full 16-row query tile carries one-hot, set and bulk rows
            per_tile = [{names[p].rstrip("0123456789") for p in c.plan_of[0, t * 16:(t + 1) * 16].tolist()} for t in range(L // 16)]
            assert all(len(s) >= 2 for s in per_tile) and sum(s >= {"onehot", "set", "bulk"} for s in per_tile) >= len(per_tile) // 2


# ----------------------------------------------------------------------------------------------------------- representability
def _is_int(t):
    return bool((t == t.round()).all())


@pytest.mark.parametrize("cs,mode", ALL, ids=ids(ALL))
def test_representability(cs, mode):
    md = A.MODES[mode]
    fp32 = lambda t: bool((t.float().double() == t).all())
    bf16 = lambda t: bool((R.bf16_rne(t).double() == t).all())
    for kind in A.KINDS:
        c = A.case(*cs, mode, kind)
        raw = c.q @ c.k.transpose(1, 2)
        # q.k is an fp32 number, and so is its scaled value (head dim 64: a power of two; set families: 2048 times the fp32 scale).
        # Moderate scores at head dims 32 / 128 round once in s * scale: the 2 SMAX U23 of allowances() covers it
        assert fp32(raw) and (fp32(c.s) or (kind == "mod" and cs[0] != 64))
        assert bool((c.n >= 1).all())
        if kind == "mod":
            top = torch.where(c.M, c.s, torch.full_like(c.s, -1e300)).amax(-1, keepdim=True)
            assert float(c.s[c.M].abs().max()) <= A.SMAX and bool(((c.s - top)[~c.M] <= -104.0).all())
            assert float(c.s[c.M].abs().max()) > 0.25 * A.SMAX      # and the scores do reach that magnitude
        else:
            assert bool((c.s[c.M] == 0).all()) and bool((c.s[~c.M] <= -104.0).all())
    c = A.case(*cs, mode, "int")
    ta = c.tier_a(mode)
    f, b, kv = ta["fwd"], ta["dq"], ta["dkv"]
    assert bool(ta["lse"].any()) and bool((f | ~ta["lse"]).all()) and bool((b | ~ta["lse"]).all())    # one-hot rows: exact everywhere
    assert bool(kv.any()) and bool((c.n[f] <= 8).all())
    if md["round"] and c.L >= 33:
        assert bool((b & (c.n > 1)).any()), "no power-of-two row has an exact backward in a mode that rounds P"
    # forward: P = 1 inside the running sums (scores 0, maximum 0 or -2048 scale), so o and l are sums of integers
    assert _is_int(c.v) and float(c.v.abs().sum(1).max()) < 2 ** 24 and c.L < 2 ** 24
    assert fp32(c.P[f]) and fp32(c.out_bh[f]) and (not md["round"] or bf16(c.P[f]))
    assert fp32(R.bf16_rne(c.out_bh[f]).double())
    # backward
    assert _is_int(c.dP) and float(c.dP.abs().max()) < 2 ** 8       # dP within 8 significant bits
    assert fp32(c.delta[b]) and _is_int(c.delta[b] * 8)
    dS = c.dS[b]
    assert _is_int(dS * 64) and (not md["round"] or bf16(dS)) and fp32(dS)
    assert not bool(((c.dS != 0) & ~c.M)[b].any())                  # dS is 0 wherever q holds -2048: the product is 0 * -2048
    assert bool((c.dS[ta["lse"]] == 0).all())                       # one-hot rows: dq = dk = 0, dv the scatter of dout
    if md["stored"]:
        assert bf16(c.out_bh[b])
    assert float(c.raw["Sdq"][b].max()) * 64 < 2 ** 24 and _is_int(c.raw["dq"][b] * 64)
    Sdk = (c.dS.abs() * b[:, :, None]).transpose(1, 2) @ c.q.abs()
    # (group band of dk: products dS * -2048, multiples of 32; the free bands: multiples of 1/64)
    assert float(Sdk[kv][:, :A.G].max()) / 32 < 2 ** 24 and float(Sdk[kv][:, A.G:].max()) * 64 < 2 ** 24 and _is_int(c.raw["dk"][kv] * 64)
    assert _is_int((c.P.transpose(1, 2) @ c.do)[kv] * 8)           # dv of an exact key: rows with P = 2^-n, n <= 3, only
    # (dq * scale, dk * scale: an integer below 2^24 in units of 1/64 times a 24-bit scale is exact in float64, so the reference's
    # .float() is the one rounding the kernel makes)


# ------------------------------------------------------------------------------------------------------------------- mutants
@pytest.mark.parametrize("cs,mode", ALL, ids=ids(ALL))
def test_unmutated_emulation_passes(cs, mode):
    for kind in A.KINDS:
        c = A.case(*cs, mode, kind)
        A.check(c, mode, A.emulate(c, mode))
    if mode == "b16":              # the result does not depend on the chunking
        c = A.case(*cs, mode, "int")
        A.check(c, mode, A.emulate(c, mode, chunk=32))


MUTANT_CASES = [((64, 33, 2, 2), "f32"), ((64, 290, 2, 2), "bf16"), ((32, 33, 2, 2), "x3"), ((64, 225, 2, 2), "b16"), ((64, 230, 2, 2), "b16")]


def _rejected(c, mode, mutant, tiers):
    try:
        A.check(c, mode, A.emulate(c, mode, mutant=mutant), tiers=tiers)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mutant", A.MUTANTS)
def test_mutants_are_rejected(mutant):
    if mutant == "p_truncated":        # shows only where P is rounded and is not a power of two: bf16 modes, fractional family
        hits = [(cs, m) for cs, m in MUTANT_CASES if A.MODES[m]["round"] and _rejected(A.case(*cs, m, "frac"), m, mutant, "B")]
        assert hits, "a truncated P passes the bounded tier"
        return
    for tiers, kind in (("A", "int"), ("B", "frac"), ("B", "mod")):
        hits = [(cs, m) for cs, m in MUTANT_CASES if _rejected(A.case(*cs, m, kind), m, mutant, tiers)]
        assert hits, f"{mutant}: tier {tiers} on the {kind} family rejects it on no case"


def test_float64_softmax_leaves_residues():
    """why the reference takes P from the sets: torch.softmax in float64 leaves non-zero weights on disallowed keys"""
    c = A.case(64, 33, 2, 2, "f32", "int")
    sm = torch.softmax(c.s, -1)
    assert bool((c.P[~c.M] == 0).all()) and bool((sm[~c.M] > 0).any())
    assert bool((c.lse[c.n == 1] == 0).all()) and torch.allclose(sm, c.P, atol=1e-100, rtol=1e-15)
