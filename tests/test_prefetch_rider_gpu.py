"""Prefetch riders (include/unetr_hip.h: unetr_prefetch): extra workgroups of the LayerNorm / attention launches that only read the
weights of the GEMM behind them.  A rider has no side effect, so everything here is a bit comparison: each host entry point with
and without a range, odd ranges, one transformer block with riders on and off, and a captured graph of that block."""
import pytest
import torch

pytestmark = pytest.mark.gpu

H, HEADS, MLP = 768, 12, 3072
ROWS = (432, 430)          # the benchmark's token rows, and a row count that is not a multiple of 4


def _pf(pkg, *ranges):
    """unetr_prefetch over (address, bytes) pairs"""
    pf = pkg._capi.Prefetch()
    for i, (p, n) in enumerate(ranges):
        pf.ptr[i], pf.bytes[i] = p, n
    return pf


def _weight(dev, nbytes=4718592 + 64):
    # exactly nbytes long: a rider that read past the end of a range would leave the allocation
    return torch.randint(0, 255, (nbytes,), dtype=torch.uint8, device=dev)


def _ranges(pkg, dev):
    """the range cases of one host launch: name -> unetr_prefetch or None.  Buffers are kept alive by the returned list."""
    w, w2, tiny = _weight(dev), _weight(dev, 1179648), _weight(dev, 64)
    p, n = w.data_ptr(), w.numel()
    cases = {
        "whole": _pf(pkg, (p, n)),
        "misaligned": _pf(pkg, (p + 2, 16 * 1000 + 6)),
        "short": _pf(pkg, (tiny.data_ptr() + 3, 15)),
        "zero": _pf(pkg, (p, 0)),
        "null": _pf(pkg, (None, 4096)),
        "two": _pf(pkg, (p, n), (w2.data_ptr(), w2.numel())),
        "two_second_only": _pf(pkg, (None, 0), (w2.data_ptr() + 6, w2.numel() - 6)),
        "to_the_end": _pf(pkg, (p + n - 16 * 4099 - 5, 16 * 4099 + 5)),
        "tiny_to_the_end": _pf(pkg, (tiny.data_ptr() + 1, 63)),
        "none": None,
    }
    return cases, [w, w2, tiny]


def _same(a, b):
    assert len(a) == len(b)
    for s, t in zip(a, b):
        assert s.dtype == t.dtype and s.shape == t.shape
        assert torch.equal(s.view(torch.uint8), t.view(torch.uint8))


def _check(pkg, dev, run):
    """run(pf) -> tuple of output tensors: every range case gives the bits of the rider-less call"""
    cases, keep = _ranges(pkg, dev)
    ref = run(None)
    for name, pf in cases.items():
        out = run(pf)
        torch.cuda.synchronize()
        try:
            _same(ref, out)
        except AssertionError as e:
            raise AssertionError(f"range case {name!r}") from e
    del keep


@pytest.mark.parametrize("M", ROWS)
def test_layernorm_fwd_rider(pkg, dev, M):
    Fn = pkg.functional
    torch.manual_seed(0)
    x, g, b = torch.randn(M, H, device=dev), torch.randn(H, device=dev), torch.randn(H, device=dev)

    def run(pf):
        yb = Fn.bf16_like(x)
        y, mean, rstd = Fn.layernorm_fwd(x, g, b, bf16_out=yb, pf=pf)
        return y, yb, mean, rstd
    _check(pkg, dev, run)


@pytest.mark.parametrize("M", ROWS)
def test_layernorm_bwd_rider(pkg, dev, M):
    Fn = pkg.functional
    torch.manual_seed(1)
    x, g, b = torch.randn(M, H, device=dev), torch.randn(H, device=dev), torch.randn(H, device=dev)
    dy, dres = torch.randn(M, H, device=dev), torch.randn(M, H, device=dev)
    _, mean, rstd = Fn.layernorm_fwd(x, g, b)

    def run(pf):
        dxb = Fn.bf16_like(x)
        dx, dw, db = Fn.layernorm_bwd(dy, x, g, mean, rstd, dres=dres, dx_bf16=dxb, pf=pf)
        return dx, dxb, dw, db
    _check(pkg, dev, run)


@pytest.mark.parametrize("M", ROWS)
def test_layernorm_fwd_slab_form_rider(pkg, dev, M):
    """LayerNorm on the split-K slabs of linear2 (unetr_gemm_bf16_ln_fwd_pf)"""
    Fn = pkg.functional
    torch.manual_seed(2)
    a = torch.randn(M, MLP, device=dev).bfloat16()
    w2 = (torch.randn(H, MLP, device=dev) * 0.02).bfloat16()
    bias, res = torch.randn(H, device=dev), torch.randn(M, H, device=dev)
    g, b = torch.randn(H, device=dev), torch.randn(H, device=dev)

    def run(pf):
        c, yb = torch.empty(M, H, device=dev), torch.empty(M, H, device=dev, dtype=torch.bfloat16)
        mean, rstd = Fn.gemm_bf16_ln_fwd(a, w2, M, H, MLP, c, g, b, yb, bias=bias, res=res, ldr=H, pf=pf)
        return c, yb, mean, rstd
    _check(pkg, dev, run)


@pytest.mark.parametrize("M", ROWS)
def test_layernorm_bwd_slab_form_rider(pkg, dev, M):
    """LayerNorm backward on the split-K slabs of linear1's data gradient (unetr_gemm_bf16_ln_bwd_pf)"""
    Fn = pkg.functional
    torch.manual_seed(3)
    du = torch.randn(M, MLP, device=dev).bfloat16()
    w1 = (torch.randn(MLP, H, device=dev) * 0.02).bfloat16()
    x, g, b = torch.randn(M, H, device=dev), torch.randn(H, device=dev), torch.randn(H, device=dev)
    dres = torch.randn(M, H, device=dev)
    _, mean, rstd = Fn.layernorm_fwd(x, g, b)

    def run(pf):
        dxb = Fn.bf16_like(x)
        dx, dw, db = Fn.gemm_ln_bwd_params(du, w1, M, H, MLP, x, g, b, mean, rstd, dres=dres, dx_bf16=dxb, pf=pf)
        return dx, dxb, dw, db
    _check(pkg, dev, run)


@pytest.mark.parametrize("L", (216, 215))     # B * L = 432 / 430 token rows
def test_attention_bf16_rider(pkg, dev, L):
    Fn = pkg.functional
    B, dh = 2, H // HEADS
    torch.manual_seed(4)
    qkv = torch.randn(B * L, 3 * H, device=dev).bfloat16()
    dout = torch.randn(B * L, H, device=dev).bfloat16()

    def fwd(pf):
        outb, out = torch.empty(B * L, H, device=dev, dtype=torch.bfloat16), torch.empty(B * L, H, device=dev)
        lse = Fn.attention_bf16_fwd(qkv, B, L, HEADS, dh, outb, out=out, pf=pf)
        return out, outb, lse
    _check(pkg, dev, fwd)
    _, outb, lse = fwd(None)

    def bwd(pf):
        dqkv = torch.empty(B * L, 3 * H, device=dev)
        dqkvb = Fn.attention_bf16_bwd(qkv, outb, dout, lse, B, L, HEADS, dh, dqkv=dqkv, pf=pf)
        return dqkv, dqkvb
    _check(pkg, dev, bwd)


class _Block:
    """one MONAI TransformerBlock's parameters + the neighbours' weights its riders name, at the benchmark's shape"""

    def __init__(self, pkg, dev):
        Fn = pkg.functional
        torch.manual_seed(5)

        def par(*shape, scale=0.02):
            return torch.nn.Parameter(torch.randn(*shape, device=dev) * scale)
        self.B, self.L = 2, 216
        self.n1w, self.n1b, self.n2w, self.n2b = par(H, scale=1.0), par(H), par(H, scale=1.0), par(H)
        self.wqkv, self.wp, self.bp = par(3 * H, H), par(H, H), par(H)
        self.w1, self.b1, self.w2, self.b2 = par(MLP, H), par(MLP), par(H, MLP), par(H)
        self.nn1w, self.nn1b = par(H, scale=1.0), par(H)                      # the next block's norm1
        self.next_wqkv, self.below_w2, self.below_w1 = par(3 * H, H), par(H, MLP), par(MLP, H)
        for w in (self.next_wqkv, self.below_w2, self.below_w1):
            Fn.weight_bf16(w)                                                # (their own blocks would have made these shadows)
        self.x = torch.randn(self.B * self.L, H, device=dev, requires_grad=True)
        self.gout = torch.randn(self.B * self.L, H, device=dev)
        self.pkg = pkg

    def params(self):
        return [self.n1w, self.n1b, self.wqkv, self.wp, self.bp, self.n2w, self.n2b, self.w1, self.b1, self.w2, self.b2]

    def run(self):
        """forward + backward: (x2, the stashed norm1 of the next block, dx, every parameter gradient)"""
        Fn = self.pkg.functional
        x2 = Fn.TransformerBlockFn.apply(self.x, *self.params(), self.B, self.L, HEADS, self.pkg._capi.PREC_BF16, False,
                                         self.nn1w.detach(), self.nn1b.detach(), False,
                                         self.next_wqkv.detach(), self.below_w2.detach(), self.below_w1.detach())
        xn, mn, rn = x2._unetr_ln[:3]
        grads = torch.autograd.grad(x2, [self.x] + self.params(), self.gout)
        return (x2.detach(), xn, mn, rn) + tuple(grads)


def test_transformer_block_riders_on_off(pkg, dev):
    Fn = pkg.functional
    blk = _Block(pkg, dev)
    blk.run()                                       # the bf16 weight shadows exist from here on
    assert Fn.PREFETCH_RIDERS
    for w in (blk.wqkv, blk.wp, blk.w1, blk.w2, blk.next_wqkv.detach(), blk.below_w2.detach(), blk.below_w1.detach()):
        pf = Fn._prefetch("ln1_fwd", w)
        assert pf is not None and pf.bytes[0] == w.numel() * 2, "the riders of this block have nothing to read"
    on = blk.run()
    try:
        Fn.PREFETCH_RIDERS = False
        assert Fn._prefetch("ln1_fwd", blk.wqkv) is None
        off = blk.run()
    finally:
        Fn.PREFETCH_RIDERS = True
    torch.cuda.synchronize()
    _same(off, on)


def test_transformer_block_riders_graph_replay(pkg, dev):
    blk = _Block(pkg, dev)
    blk.run()
    eager = [t.clone() for t in blk.run()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        blk.run()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = blk.run()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    _same(eager, outs)
