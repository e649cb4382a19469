"""Transposed bf16 weight shadow (functional.weight_bf16_t): the fused weight-gradient + AdamW epilogue that writes it, the grouped
derive launch, the four ViT data gradients in the forward kernel form on it, and its freshness under every kind of weight update."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from util import relerr

pytestmark = pytest.mark.gpu

SENTINEL = 0x7B5A          # bit pattern no test weight rounds to (bf16 2.8e35)


def g(*shape, seed=0, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=gen) * scale


def _bits(t):
    return t.view(torch.int16)


def test_fused_epilogue_writes_transposed_shadow(pkg, dev):
    """(a) unetr_gemm_bf16_grouped_wgrad_adamw_t with shadow_t set: params, both moments and the bf16 shadow bit-identical to the run
    with shadow_t = NULL over two optimizer steps; every weight's shadow_t slice == shadow.view(N, K).t() bit for bit; every other byte
    of the sentinel-filled shadow_t untouched.  Shapes of test_grouped_wgrad_fused_epilogues (ragged N, K, gaps between the matrices)."""
    capi = pkg._capi
    st = torch.cuda.current_stream().cuda_stream
    shapes = [(432, 768, 256), (216, 200, 136), (64, 8, 8), (432, 128, 384)]
    gaps = (48, 8, 0, 24)
    offs, total = [], 40
    for (_, N, K), gap in zip(shapes, gaps):
        offs.append(total)
        total += N * K + gap
    torch.manual_seed(5)
    p0 = (torch.randn(total) * 0.05).to(dev)
    ops = [(g(M, N, seed=30 + i).bfloat16().to(dev), g(M, K, seed=40 + i).bfloat16().to(dev)) for i, (M, N, K) in enumerate(shapes)]

    def run(with_t):
        p, m, v = p0.clone(), torch.zeros(total, device=dev), torch.zeros(total, device=dev)
        grad = torch.zeros(total, device=dev)
        shadow = torch.zeros(total, device=dev, dtype=torch.bfloat16)
        twin = torch.full((total,), SENTINEL, device=dev, dtype=torch.int16)
        steps = torch.zeros(len(shapes), device=dev)
        steps[1] = 3.0
        arr = (capi.GroupedProblem * len(shapes))()
        for i, ((dy, x), (M, N, K)) in enumerate(zip(ops, shapes)):
            arr[i].dy, arr[i].x, arr[i].dw = dy.data_ptr(), x.data_ptr(), grad.data_ptr() + 4 * offs[i]
            arr[i].M, arr[i].N, arr[i].K = M, N, K
        sidx = (ctypes.c_int * len(shapes))(*range(len(shapes)))
        for _ in range(2):
            steps += 1.0
            arena = capi.AdamWArena(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), shadow.data_ptr(), steps.data_ptr(), total,
                                    1e-3, 0.9, 0.999, 1e-8, 1e-2)
            capi.call("unetr_gemm_bf16_grouped_wgrad_adamw_t", arr, len(shapes), ctypes.byref(arena), sidx,
                      twin.data_ptr() if with_t else None, st)
        torch.cuda.synchronize()
        return p, m, v, shadow, twin

    ref, new = run(False), run(True)
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq", "shadow"), ref, new):
        assert torch.equal(a, b), name
    assert (ref[0] != p0).float().mean() > 0.9                      # the weights moved
    assert (ref[4] == SENTINEL).all()                               # shadow_t = NULL: nothing written anywhere
    shadow, twin = new[3], new[4]
    outside = torch.ones(total, dtype=torch.bool, device=dev)
    for (_, N, K), o in zip(shapes, offs):
        want = _bits(shadow[o:o + N * K]).view(N, K).t().contiguous()
        assert torch.equal(twin[o:o + N * K].view(K, N), want), (N, K)
        outside[o:o + N * K] = False
    assert (twin[outside] == SENTINEL).all()


def test_transpose_grouped_derive_launch(pkg, dev):
    """(b) unetr_transpose_bf16_grouped against torch.t() at four shapes (one tile corner, ragged, the two large ViT shapes) in ONE
    grouped call; bytes outside the slices untouched"""
    capi = pkg._capi
    shapes = [(8, 8), (200, 136), (768, 3072), (2304, 768)]
    gaps = (8, 24, 0, 16)
    offs, total = [], 16
    for (N, K), gap in zip(shapes, gaps):
        offs.append(total)
        total += N * K + gap
    src = g(total, seed=3).bfloat16().to(dev)
    dst = torch.full((total,), SENTINEL, device=dev, dtype=torch.int16)
    arr = (capi.TransposeProblem * len(shapes))()
    for i, ((N, K), o) in enumerate(zip(shapes, offs)):
        arr[i].offset, arr[i].N, arr[i].K = o, N, K
    capi.call("unetr_transpose_bf16_grouped", src.data_ptr(), dst.data_ptr(), arr, len(shapes), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    outside = torch.ones(total, dtype=torch.bool, device=dev)
    for (N, K), o in zip(shapes, offs):
        assert torch.equal(dst[o:o + N * K].view(K, N), _bits(src[o:o + N * K]).view(N, K).t().contiguous()), (N, K)
        outside[o:o + N * K] = False
    assert (dst[outside] == SENTINEL).all()


# (c) the four data gradients of a transformer block, dx[M, in] = dy[M, out] . W[out, in]: (name, out, in, epilogue)
def _dgrad_shapes(hid, mlp):
    return [("du", hid, mlp, "gelu"), ("datt", hid, hid, None), ("dy2", mlp, hid, "ln"), ("dx", 3 * hid, hid, "ln")]


@pytest.mark.parametrize("hid,mlp,M", [(128, 512, 72), (128, 512, 432), (768, 3072, 432)])
def test_dgrad_forward_form_on_twin_equals_bkn_form(pkg, dev, hid, mlp, M):
    """(c) NT-on-Wt and b_kn-on-W, with the tile and split-K choice the dispatcher makes for each: both under the bf16 GEMM bound
    (relerr < 2e-5, as test_gemm_bf16_grouped_wgrad) against the fp64 product of the same bf16 inputs, and bit-equal to each other
    (the step forms that read the twin and those that do not are held bit for bit by test_staged_backward_equals_single_pass).
    With the GELU' epilogue (du, fp32 and bf16 outputs) and the LayerNorm-riding form (dy2, dx: the output is LayerNorm backward of
    the product), under the same 2e-5."""
    Fn = pkg.functional
    for i, (name, out, inn, ep) in enumerate(_dgrad_shapes(hid, mlp)):
        dy = g(M, out, seed=10 + i).bfloat16()
        w = g(out, inn, seed=20 + i, scale=0.05).bfloat16()
        prod = dy.double() @ w.double()
        dyd, wd = dy.to(dev), w.to(dev)
        wt = wd.t().contiguous()
        c_t, c_k = torch.empty(M, inn, device=dev), torch.empty(M, inn, device=dev)
        Fn.gemm_bf16(dyd, wt, M, inn, out, C=c_t)
        Fn.gemm_bf16(dyd, wd, M, inn, out, b_kn=True, C=c_k)
        e_t, e_k, same = relerr(c_t, prod), relerr(c_k, prod), torch.equal(c_t, c_k)
        print(f"{name} [{M} x {inn}] K={out}: NT-on-Wt {e_t:.2e}  b_kn {e_k:.2e}  bit-equal {same}")
        assert e_t < 2e-5 and e_k < 2e-5, name
        assert same, name
        if ep == "gelu":
            u = g(M, inn, seed=30 + i)
            ur = u.clone().requires_grad_(True)
            F.gelu(ur).sum().backward()
            ud = u.to(dev)
            b_t, b_k = (torch.empty(M, inn, device=dev, dtype=torch.bfloat16) for _ in range(2))
            Fn.gemm_bf16(dyd, wt, M, inn, out, C=c_t, Cb=b_t, act=2, aux=ud, ldaux=inn)
            Fn.gemm_bf16(dyd, wd, M, inn, out, b_kn=True, C=c_k, Cb=b_k, act=2, aux=ud, ldaux=inn)
            ref = prod * ur.grad.double()
            e_t, e_k, same = relerr(c_t, ref), relerr(c_k, ref), torch.equal(c_t, c_k) and torch.equal(b_t, b_k)
            print(f"{name} + GELU': NT-on-Wt {e_t:.2e}  b_kn {e_k:.2e}  bit-equal {same}")
            assert e_t < 2e-5 and e_k < 2e-5 and same, name
        if ep == "ln":
            x, gam, bet, dres = g(M, inn, seed=40 + i) * 2 + 0.5, g(inn, seed=50 + i), g(inn, seed=60 + i), g(M, inn, seed=70 + i)
            xr, gr, br = x.double().requires_grad_(True), gam.double().requires_grad_(True), bet.double().requires_grad_(True)
            F.layer_norm(xr, (inn,), gr, br, 1e-5).backward(prod)
            xd, gd, bd, dd = x.to(dev), gam.to(dev), bet.to(dev), dres.to(dev)
            _, mean, rstd = Fn.layernorm_fwd(xd, gd, bd)
            outs = []
            for B, bkn in ((wt, False), (wd, True)):
                dxb = torch.empty(M, inn, device=dev, dtype=torch.bfloat16)
                dx, dgam, dbet = Fn.gemm_ln_bwd_params(dyd, B, M, inn, out, xd, gd, bd, mean, rstd, dres=dd, dx_bf16=dxb, b_kn=bkn)
                outs.append((dx, dgam, dbet, dxb))
            same = all(torch.equal(a, b) for a, b in zip(*outs))
            errs = [(relerr(o[0], xr.grad + dres.double()), relerr(o[1], gr.grad), relerr(o[2], br.grad)) for o in outs]
            print(f"{name} LayerNorm-riding: NT-on-Wt {errs[0]}  b_kn {errs[1]}  bit-equal {same}")
            assert max(errs[0]) < 2e-5 and max(errs[1]) < 2e-5 and same, name


C1 = dict(in_channels=1, out_channels=2, img_size=(32, 32, 32), feature_size=16, hidden_size=128, mlp_dim=512,
          num_heads=4, pos_embed="perceptron", norm_name="instance", res_block=True)


def _linear_weights(m):
    for blk in m.vit.blocks:
        yield from (blk.attn.qkv.weight, blk.attn.out_proj.weight, blk.mlp.linear1.weight, blk.mlp.linear2.weight)


def _twins_match(pkg, m, flat, stamped):
    """every block's twin == its transposed bf16 shadow, bit for bit, in the arenas themselves (no getter in between); stamped: the
    table also vouches for them (forms that run Python every step)"""
    Fn = pkg.functional
    torch.cuda.synchronize()
    index = {id(p): o for p, o in zip(flat["params"], flat["offsets"])}
    for w in _linear_weights(m):
        o, (N, K) = index[id(w)], w.shape
        want = _bits(flat["shadow"][o:o + N * K]).view(N, K).t().contiguous()
        assert torch.equal(_bits(flat["shadow_t"][o:o + N * K]).view(K, N), want), (N, K)
        assert torch.equal(flat["shadow"][o:o + N * K].view(N, K), w.detach().bfloat16())
        if stamped:
            assert Fn.twin_at(w) is not None


def _takes_twin_route(pkg, m):
    """what a backward pass reads for every block weight now: the twin, in the forward form"""
    Fn = pkg.functional
    for w in _linear_weights(m):
        B, bkn = Fn._dgrad_operand(w, 16)
        assert bkn is False and B.data_ptr() == Fn.twin_at(w).data_ptr() and B.shape == (w.shape[1], w.shape[0])
        assert Fn._dgrad_operand(w, Fn.WT_MAX_ROWS + 8)[1] is True          # (above the measured range: the b_kn form)


def _model(pkg, dev, seed=11):
    from oracle.unetr_oracle import synthetic_volume
    torch.manual_seed(seed)
    m = pkg.UNETRLogits(**C1).to(dev)
    m.precision = "bf16"
    flat = m.use_flat_buffers()
    opt = pkg.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-5, flat=flat)
    x, y = synthetic_volume(2, 1, 32, 2, seed=41)
    return m, flat, opt, x.to(dev), y.to(dev), pkg.DiceCELoss(to_onehot_y=True, softmax=True)


def _disturb(pkg, m, kind):
    if kind == "inplace":
        with torch.no_grad():
            m.vit.blocks[1].mlp.linear1.weight.mul_(1.25)
    elif kind == "load_state_dict":
        m.load_state_dict({k: v.clone() * 0.9 for k, v in m.state_dict().items()}, strict=True)
    elif kind == "data":
        m.vit.blocks[2].attn.qkv.weight.data.mul_(0.5)
        pkg.invalidate_weight_shadows()


@pytest.mark.parametrize("form", ["fused_graph", "fused_eager", "unfused"])
def test_twin_freshness(pkg, dev, form, monkeypatch):
    """(d) C1-size model, flat arenas, bf16 mode: three steps in the fused graph form, the eager fused form and the unfused arena
    step; after every step each block's Wt equals its transposed bf16 shadow bit for bit -- also after an in-place torch op on one
    weight, after load_state_dict, and after p.data.mul_() + invalidate_weight_shadows().  With UNETR_AMD_WT=0 no twin arena exists and
    the losses of the three steps agree with the feature on to 2e-4 (the suite's bound on a bf16 step's loss, C2_BOUNDS in
    test_model_gpu.py; the two kernel forms give the same bits, so they are in fact equal)."""
    def steps(wt_on):
        monkeypatch.setenv("UNETR_AMD_WT", "1" if wt_on else "0")
        m, flat, opt, x, y, crit = _model(pkg, dev)
        losses = []
        if form == "unfused":
            # (the twin arena only comes into being under a fused step: one eager fused step first, then plain arena steps)
            step = pkg.TrainStep(m, crit, opt, x, y, use_graph=False, warmup=2, fuse_update=True)
            del step

            def one():
                loss = crit(m(x), y)
                loss.backward()
                opt.step()
                opt.zero_grad(set_to_none=True)
                return float(loss.detach())
        else:
            step = pkg.TrainStep(m, crit, opt, x, y, use_graph=form == "fused_graph", warmup=2, fuse_update=True)
            assert step.fuse and (step.graphs is not None) == (form == "fused_graph")

            def one():
                step.run()
                return float(step.loss.detach())
        assert (flat.get("shadow_t") is not None) == wt_on
        if wt_on:               # after warm-up (and capture) the backward pass reads the twins, not the b_kn form
            _takes_twin_route(pkg, m)
        for kind in (None, None, None, "inplace", "load_state_dict", "data"):
            if kind is not None:
                _disturb(pkg, m, kind)
            losses.append(one())
            if wt_on:
                _twins_match(pkg, m, flat, stamped=form != "fused_graph")
        flat["state"].clear()
        return losses

    on, off = steps(True), steps(False)
    print(form, "losses with the twin:", on[:3], "without:", off[:3], "equal:", on == off)
    for a, b in zip(on[:3], off[:3]):
        assert abs(a - b) <= 2e-4 * abs(b)


def test_captured_unfused_step_after_fused_step(pkg, dev, monkeypatch):
    """A step captured into a graph whose optimizer part does not write the twin must not read it: one eager fused step creates
    the twins, then the unfused step and the one-graph overlap_update step are captured on the same model and replayed four times;
    parameters and losses equal those of the same sequence with UNETR_AMD_WT=0 bit for bit (with a twin baked into such a graph
    they would drift from the second replay on: nothing in the graph rewrites it)."""
    Fn = pkg.functional

    def run(wt_on, overlap):
        monkeypatch.setenv("UNETR_AMD_WT", "1" if wt_on else "0")
        m, flat, opt, x, y, crit = _model(pkg, dev)
        pkg.TrainStep(m, crit, opt, x, y, use_graph=False, warmup=2, fuse_update=True)        # eager: unfused step, fused step
        assert (flat.get("shadow_t") is not None) == wt_on
        step = pkg.TrainStep(m, crit, opt, x, y, use_graph=True, warmup=1, fuse_update=False, overlap_update=overlap)
        assert step.graphs is not None and len(step.graphs) == 1
        if wt_on:              # under capture no twin was handed out: whatever the table says now, the graph holds b_kn launches
            st = flat["state"]
            assert st.fuse is None
        losses = []
        for _ in range(4):
            step.run()
            losses.append(float(step.loss.detach()))
        torch.cuda.synchronize()
        out = (flat["param"].clone(), losses)
        flat["state"].clear()
        return out

    for overlap in (False, True):
        on, off = run(True, overlap), run(False, overlap)
        print("overlap_update" if overlap else "unfused graph", "losses:", on[1], off[1])
        assert on[1] == off[1] and torch.equal(on[0], off[0]), overlap
