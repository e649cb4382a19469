"""Gradient clipping by global norm on the device (csrc/grad_clip.hip, optim.AdamW(max_grad_norm=...), TrainStep, clip_grad_norm_).

Kernel level: the norm against a float64 sum of the same bits (1 fp32 ulp), run-to-run reproducibility, inf / NaN, the fp32
coefficient bit for bit, a captured two-launch graph following unetr_grad_clip_set, and unetr_adamw_hyper_clip bit for bit against
unetr_adamw_hyper on pre-scaled gradients.  Model level (C1 geometry of tests/test_lr_schedule_gpu.py: 32^3, hidden 128, 4 heads,
batch 2): max_grad_norm = inf changes no bit in any launch form, a finite threshold equals scaling the arena by hand, every captured /
overlapped / data-parallel form equals the eager clipped step, the refusals, and the free function on ordinary tensors."""
import numpy as np
import pytest
import torch

import grad_clip_ref as R

pytestmark = pytest.mark.gpu

C1 = dict(in_channels=1, out_channels=2, img_size=(32, 32, 32), feature_size=16, hidden_size=128, mlp_dim=512,
          num_heads=4, pos_embed="perceptron", norm_name="instance", res_block=True)
LR, WD, B1, B2, EPS = 1e-3, 1e-2, 0.9, 0.999, 1e-8
LENGTHS = [1, 3, 4, 5, 4095, 4096, 4097, 65537]
BLOCK = 8192


def g(*shape, seed=0, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=gen) * scale


def stream():
    return torch.cuda.current_stream().cuda_stream


def new_row(dev, max_norm):
    return torch.tensor([0.0, 1.0, max_norm, 0.0], dtype=torch.float32, device=dev)


def torch_coef(norm, max_norm):
    """the fp32 expression of torch.nn.utils.clip_grad_norm_ on a float32 norm (CPU tensors)"""
    n = torch.tensor(float(norm), dtype=torch.float32)
    return torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (n + 1e-6), max=1.0)


def same_bits(a, b):
    return np.float32(a).view(np.int32) == np.float32(b).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------- kernel level
def _ranges_buffer(dtype, dev):
    """a flat buffer with the ranges of LENGTHS at offsets that are multiples of 8, every gap filled with NaN and 1e30 alternately;
    seeded normals with per-range scales 2^-20 .. 2^20.  Returns (buffer, rows (lo, hi, first_block), blocks)."""
    rows, o, blocks = [], 8, 0
    for n in LENGTHS:
        rows.append((o, o + n, blocks))
        blocks += (n + BLOCK - 1) // BLOCK
        o = (o + n + 7) // 8 * 8 + 8
    buf = torch.empty(o, dtype=torch.float32)
    buf[0::2] = float("nan")
    buf[1::2] = 1e30
    for k, ((lo, hi, _), n) in enumerate(zip(rows, LENGTHS)):
        buf[lo:hi] = g(n, seed=100 + k, scale=2.0 ** (-20 + 40 * k / (len(LENGTHS) - 1)))
    return buf.to(dtype).to(dev), rows, blocks


@pytest.mark.parametrize("gscale", [1.0, 1.0 / 8, 1.0 / 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_norm_over_ranges(pkg, dev, dtype, gscale):
    capi = pkg._capi
    buf, rows, blocks = _ranges_buffer(dtype, dev)
    table = torch.tensor(rows, dtype=torch.int64, device=dev)
    host = buf.float().cpu().numpy()
    want = R.norm_f32([host[lo:hi] for lo, hi, _ in rows], gscale)
    assert np.isfinite(want) and want > 0
    out = []
    for _ in range(2):
        part = torch.full((blocks + 2,), -7.0, dtype=torch.float64, device=dev)
        row = new_row(dev, 12.0)
        capi.call("unetr_grad_sumsq_ranges", buf.data_ptr(), int(dtype == torch.bfloat16), table.data_ptr(), len(rows), blocks,
                  part.data_ptr(), blocks * 8, stream())
        capi.call("unetr_grad_clip_finalize", part.data_ptr(), blocks, gscale, row.data_ptr(), stream())
        out.append((row.cpu(), part.cpu()))
    (row, part), (row2, part2) = out
    norm = row[0].item()
    print(f"{dtype} gscale {gscale}: device norm {norm!r}, float64 reference {float(want)!r}, ulps {R.ulp_diff(norm, want)}")
    assert R.ulp_diff(norm, want) <= 1
    assert torch.equal(row, row2) and torch.equal(part, part2)                    # bitwise reproducible, partials included
    assert part[blocks:].tolist() == [-7.0, -7.0] and bool((part[:blocks] >= 0).all())      # one slot per block, nothing beyond
    assert same_bits(row[1].item(), torch_coef(norm, 12.0).item()) and row[2].item() == 12.0 and row[3].item() == 0.0
    # a too small workspace is refused, not overrun
    with pytest.raises(RuntimeError, match="unetr_grad_sumsq_ranges failed"):
        capi.call("unetr_grad_sumsq_ranges", buf.data_ptr(), int(dtype == torch.bfloat16), table.data_ptr(), len(rows), blocks,
                  part.data_ptr(), blocks * 8 - 8, stream())
    # the per-tensor form, at element offsets that are NOT 16-byte aligned: the neighbours (NaN / 1e30) are not read
    lo, hi, _ = rows[-1]
    for a, b in ((lo + 1, hi), (lo + 3, hi - 2), (lo + 5, lo + 6), (lo + 2, lo + 9)):
        view = buf[a:b]
        nb = (b - a + BLOCK - 1) // BLOCK
        part = torch.zeros(nb, dtype=torch.float64, device=dev)
        row = new_row(dev, 12.0)
        capi.call("unetr_grad_sumsq", view.data_ptr(), int(dtype == torch.bfloat16), b - a, part.data_ptr(), nb * 8, stream())
        capi.call("unetr_grad_clip_finalize", part.data_ptr(), nb, gscale, row.data_ptr(), stream())
        assert R.ulp_diff(row[0].item(), R.norm_f32([host[a:b]], gscale)) <= 1, (a - lo, b - lo)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_norm_nonfinite(pkg, dev, dtype):
    """sixteen elements of 3e38: norm = inf, coef = 0, counter 1; then one NaN element: NaN norm, NaN coef, counter 2"""
    capi = pkg._capi
    buf = torch.zeros(64, dtype=torch.float32)
    buf[8:24] = 3e38
    buf = buf.to(dtype).to(dev)
    table = torch.tensor([(8, 24, 0), (32, 37, 1)], dtype=torch.int64, device=dev)
    part = torch.zeros(2, dtype=torch.float64, device=dev)
    row = new_row(dev, 12.0)

    def run():
        capi.call("unetr_grad_sumsq_ranges", buf.data_ptr(), int(dtype == torch.bfloat16), table.data_ptr(), 2, 2, part.data_ptr(), 16, stream())
        capi.call("unetr_grad_clip_finalize", part.data_ptr(), 2, 1.0, row.data_ptr(), stream())
        return row.cpu().tolist()

    norm, coef, mx, cnt = run()
    assert norm == float("inf") and coef == 0.0 and mx == 12.0 and cnt == 1.0
    buf[34] = float("nan")
    norm, coef, mx, cnt = run()
    assert np.isnan(norm) and np.isnan(coef) and mx == 12.0 and cnt == 2.0


def test_coefficient_and_captured_threshold(pkg, dev):
    """coef = the fp32 torch expression on the device norm, bit for bit: norm below, equal to, above max_norm and max_norm = inf;
    a captured norm + finalize graph replays to the threshold unetr_grad_clip_set wrote after the capture."""
    capi = pkg._capi
    vals = g(5000, seed=7, scale=0.3).to(dev)
    table = torch.tensor([(0, 5000, 0)], dtype=torch.int64, device=dev)
    part = torch.zeros(1, dtype=torch.float64, device=dev)
    row = new_row(dev, 1.0)

    def launch():
        capi.call("unetr_grad_sumsq_ranges", vals.data_ptr(), 0, table.data_ptr(), 1, 1, part.data_ptr(), 8, stream())
        capi.call("unetr_grad_clip_finalize", part.data_ptr(), 1, 1.0, row.data_ptr(), stream())

    launch()
    norm = row[0].item()
    assert R.ulp_diff(norm, R.norm_f32([vals.cpu().numpy()])) <= 1
    seen = set()
    for mx in (norm * 4.0, norm * (1.0 + 1e-6), norm, norm * 0.999999, norm * 0.5, norm / 3.0, 1e-3, float("inf")):
        capi.call("unetr_grad_clip_set", row.data_ptr(), mx, stream())
        launch()
        got = row.cpu()
        want = torch_coef(got[0].item(), mx).item()
        print(f"max_norm {mx!r}: norm {got[0].item()!r} coef {got[1].item()!r} torch {want!r}")
        assert got[0].item() == norm and same_bits(got[1].item(), want) and got[2].item() == R.f32(mx)
        seen.add(got[1].item() < 1.0)
    assert seen == {True, False} and row[3].item() == 0.0
    with pytest.raises(RuntimeError, match="unetr_grad_clip_set failed"):
        capi.call("unetr_grad_clip_set", row.data_ptr(), 0.0, stream())
    # captured: the threshold is read when the finalize kernel RUNS
    capi.call("unetr_grad_clip_set", row.data_ptr(), norm * 0.5, stream())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        launch()
    graph.replay()
    assert same_bits(row[1].item(), torch_coef(norm, norm * 0.5).item()) and row[1].item() < 0.51
    capi.call("unetr_grad_clip_set", row.data_ptr(), norm * 0.25, stream())
    graph.replay()
    assert same_bits(row[1].item(), torch_coef(norm, norm * 0.25).item()) and row[1].item() < 0.26
    capi.call("unetr_grad_clip_set", row.data_ptr(), float("inf"), stream())
    graph.replay()
    assert row.cpu().tolist() == [norm, 1.0, float("inf"), 0.0]


@pytest.mark.parametrize("g_bf16", [False, True])
@pytest.mark.parametrize("n", [1, 7, 1024, 4099, 70001])
def test_adamw_hyper_clip_equals_prescaled(pkg, dev, n, g_bf16):
    """unetr_adamw_hyper_clip(g, gscale, coef) = unetr_adamw_hyper(gscale = 1) on gradients pre-scaled in torch as (g * gscale) * coef
    in fp32: masters, both moments, the bf16 shadow and the word shadow, bit for bit, two steps on the same state."""
    capi = pkg._capi
    p0 = g(n, seed=1, scale=0.05).to(dev)
    grads = [g(n, seed=2 + i, scale=0.01).to(dev) for i in range(2)]
    if g_bf16:
        grads = [x.bfloat16() for x in grads]
    hyper = torch.tensor([LR, WD, 0.0, 0.0], dtype=torch.float32, device=dev)

    def run(clip, gscale, coef):
        p, m, v = p0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        sh, wo = torch.zeros(n, device=dev, dtype=torch.bfloat16), torch.zeros(n, device=dev, dtype=torch.int32)
        row = torch.tensor([0.0, coef, 12.0, 0.0], dtype=torch.float32, device=dev)
        for grad, count in zip(grads, (1.0, 2.0)):
            step = torch.tensor([count], dtype=torch.float32, device=dev)
            if clip:
                capi.call("unetr_adamw_hyper_clip", p.data_ptr(), grad.data_ptr(), int(g_bf16), gscale, m.data_ptr(), v.data_ptr(), n,
                          hyper.data_ptr(), B1, B2, EPS, step.data_ptr(), sh.data_ptr(), wo.data_ptr(), row.data_ptr() + 4, stream())
            else:
                pre = (grad.float() * torch.tensor(gscale, dtype=torch.float32, device=dev)) * row[1]
                assert pre.dtype == torch.float32
                capi.call("unetr_adamw_hyper", p.data_ptr(), pre.data_ptr(), 0, 1.0, m.data_ptr(), v.data_ptr(), n,
                          hyper.data_ptr(), B1, B2, EPS, step.data_ptr(), sh.data_ptr(), wo.data_ptr(), stream())
        torch.cuda.synchronize()
        return p, m, v, sh, wo

    for gscale in (1.0, 1.0 / 3):
        for coef in (0.37109375 + 1e-3, 1.0):
            ref, new = run(False, gscale, coef), run(True, gscale, coef)
            for name, a, b in zip(("param", "exp_avg", "exp_avg_sq", "shadow", "words"), ref, new):
                assert torch.equal(a, b), (name, gscale, coef)
            assert (new[0] != p0).float().mean() > 0.99
    with pytest.raises(RuntimeError, match="unetr_adamw_hyper_clip failed"):      # a missing coefficient is an error, not the unclipped form
        step = torch.ones(1, device=dev)
        capi.call("unetr_adamw_hyper_clip", p0.data_ptr(), grads[0].data_ptr(), int(g_bf16), 1.0, p0.data_ptr(), p0.data_ptr(), n,
                  hyper.data_ptr(), B1, B2, EPS, step.data_ptr(), None, None, None, stream())


def test_scale_kernels(pkg, dev):
    """unetr_grad_scale_ranges / unetr_grad_scale: g * coef inside the ranges, every byte outside untouched; coef = 1 writes nothing"""
    capi = pkg._capi
    buf, rows, blocks = _ranges_buffer(torch.float32, dev)
    table = torch.tensor(rows, dtype=torch.int64, device=dev)
    for coef in (0.4321, 1.0):
        row = torch.tensor([0.0, coef, 12.0, 0.0], dtype=torch.float32, device=dev)
        want = buf.clone()
        for lo, hi, _ in rows:
            want[lo:hi] = buf[lo:hi] * row[1]
        got = buf.clone()
        capi.call("unetr_grad_scale_ranges", got.data_ptr(), table.data_ptr(), len(rows), blocks, row.data_ptr() + 4, stream())
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        lo, hi, _ = rows[-1]
        got = buf.clone()
        want = buf.clone()
        want[lo + 3:hi - 2] = buf[lo + 3:hi - 2] * row[1]
        capi.call("unetr_grad_scale", got[lo + 3:hi - 2].data_ptr(), hi - lo - 5, row.data_ptr() + 4, stream())
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ----------------------------------------------------------------------------------------------------------------- model level
_DATA = {}


def _data(dev):
    if "xy" not in _DATA:
        from oracle.unetr_oracle import synthetic_volume
        x, y = synthetic_volume(2, 1, 32, 2, seed=41)
        _DATA["xy"] = (x.to(dev), y.to(dev))
    return _DATA["xy"]


def _build(pkg, dev, max_grad_norm):
    torch.manual_seed(11)
    m = pkg.UNETRLogits(**C1).to(dev)
    m.precision = "bf16"
    flat = m.use_flat_buffers()
    opt = pkg.AdamW(m.parameters(), lr=LR, weight_decay=1e-5, flat=flat, max_grad_norm=max_grad_norm)
    return m, flat, opt, pkg.DiceCELoss(to_onehot_y=True, softmax=True)


def _step_kwargs(mode):
    return dict(use_graph=not mode.endswith("_eager") and mode != "eager", data_parallel=mode.startswith("dp"),
                comm_dtype=torch.bfloat16 if "bf16" in mode else torch.float32, overlap_update=mode == "overlap",
                handover="stream" if "streamwait" in mode else "host")


def _snap(flat, opt, step):
    torch.cuda.synchronize()
    out = dict(param=flat["param"].clone(), exp_avg=opt._flat_state[0].clone(), exp_avg_sq=opt._flat_state[1].clone(),
               shadow=flat["shadow"].clone(), loss=float(step.loss.detach()))
    if opt.max_grad_norm is not None:
        out["norm"], out["coef"] = float(opt.grad_norm()), float(opt.clip_coef())
    return out


def _run(pkg, dev, mode, max_grad_norm, nsteps, change=None, warmup=2):
    """TrainStep in launch form `mode`; the state after the constructor's warm-up steps and after each of `nsteps` run() calls.
    change = (k, value): set_max_grad_norm(value) before run() number k (0-based)."""
    xd, yd = _data(dev)
    m, flat, opt, crit = _build(pkg, dev, max_grad_norm)
    step = pkg.TrainStep(m, crit, opt, xd, yd, warmup=warmup, **_step_kwargs(mode))
    if mode == "captured":
        assert len(step.graphs) == 1 and not step.dp
    if mode == "overlap":
        assert step.one_graph and len(step.graphs) == 1
    if mode.startswith("dp") and not mode.endswith("_eager"):
        assert len(step.graphs) == 4
    if mode.startswith("dp_bf16"):
        assert step.fuse_comm and step._comm_fuse is not None
    assert ("clipped by global norm" in step.launch) == (max_grad_norm is not None)
    out = [_snap(flat, opt, step)]
    for k in range(nsteps):
        if change is not None and change[0] == k:
            opt.set_max_grad_norm(change[1])
        step.run()
        out.append(_snap(flat, opt, step))
    if max_grad_norm is not None:
        assert opt.nonfinite_steps() == 0
    flat["state"].clear()
    return out


def _assert_same(a, b, what):
    assert len(a) == len(b)
    for k, (u, v) in enumerate(zip(a, b)):
        for name in ("param", "exp_avg", "exp_avg_sq", "shadow"):
            assert torch.equal(u[name], v[name]), (what, k, name)
        if k:          # (entry 0 is the state after the constructor: a captured step's loss tensor is first written by a replay)
            assert u["loss"] == v["loss"], (what, k, "loss")


@pytest.mark.parametrize("mode", ["eager", "captured", "overlap", "dp", "dp_eager", "dp_bf16"])
def test_inf_threshold_changes_no_bit(pkg, dev, mode):
    """(a) max_grad_norm = inf against the same launch form without clipping, after each of 3 steps: masters, moments, shadow and
    loss bit for bit -- multiplying by coef == 1 and holding the data-parallel AdamW launches back until the last piece has been
    reduced change nothing.  The reported norm is finite and positive, the coefficient 1."""
    off, on = _run(pkg, dev, mode, None, 3), _run(pkg, dev, mode, float("inf"), 3)
    _assert_same(off, on, mode)
    assert not torch.equal(on[0]["param"], on[3]["param"])
    for s in on:
        assert np.isfinite(s["norm"]) and s["norm"] > 0 and s["coef"] == 1.0


def _first_norm(pkg, dev):
    """the gradient norm of the first step, as a max_grad_norm = inf run reports it"""
    if "first_norm" not in _DATA:
        _DATA["first_norm"] = _run(pkg, dev, "eager", float("inf"), 0, warmup=1)[0]["norm"]
    return _DATA["first_norm"]


def test_finite_threshold_equals_scaling_by_hand(pkg, dev):
    """(b) max_norm = half the norm an inf run measured; 3 eager clipped steps against an identically seeded model stepped with the
    existing pieces: forward, loss, backward, flat["grad"].mul_(coef) with the coefficient the clipped run reported for that step,
    unclipped opt.step().  Masters and moments bit for bit; every reported norm within 1 ulp of the float64 norm of that step's
    gradient slices; every coef < 1."""
    max_norm = 0.5 * _first_norm(pkg, dev)
    xd, yd = _data(dev)
    m, flat, opt, crit = _build(pkg, dev, max_norm)
    step = pkg.TrainStep(m, crit, opt, xd, yd, use_graph=False, warmup=1)
    clipped, grads = [], []
    for k in range(3):
        if k:
            step.run()
        clipped.append(_snap(flat, opt, step))
        grads.append(flat["grad"].clone())
    flat["state"].clear()
    del step, opt, m, flat

    m, flat, opt, crit = _build(pkg, dev, None)
    for k in range(3):
        loss = crit(m(xd), yd)
        loss.backward()
        pattern = [p.grad is not None for p in flat["params"]]
        assert not all(pattern) and sum(pattern) > 100          # (MONAI's unused cls_token has no gradient: its slice is not counted)
        host = grads[k].cpu().numpy()
        want = R.norm_f32([host[o:o + p.numel()] for p, o, has in zip(flat["params"], flat["offsets"], pattern) if has])
        got = clipped[k]
        print(f"step {k}: reported norm {got['norm']!r}, float64 {float(want)!r}, coef {got['coef']!r}")
        assert torch.equal(flat["grad"], grads[k])              # the clipped run saw the same gradients and did not rewrite them
        assert R.ulp_diff(got["norm"], want) <= 1
        assert got["coef"] < 1.0 and same_bits(got["coef"], R.coef_f32(got["norm"], max_norm))
        flat["grad"].mul_(got["coef"])
        opt.step()
        opt.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        for name, t in (("param", flat["param"]), ("exp_avg", opt._flat_state[0]), ("exp_avg_sq", opt._flat_state[1])):
            assert torch.equal(t, got[name]), (k, name)
    flat["state"].clear()


_CLIPPED = {}


def _clipped_run(pkg, dev, mode):
    base = _first_norm(pkg, dev)
    return _run(pkg, dev, mode, 0.5 * base, 4, change=(2, 0.25 * base))


@pytest.mark.parametrize("mode", ["captured", "overlap", "dp", "dp_streamwait", "dp_eager"])
def test_launch_forms_equal_eager_clipped(pkg, dev, mode):
    """(c) 4 replays with set_max_grad_norm between replays 2 and 3: every captured / overlapped / data-parallel fp32 form equals the
    eager clipped run bit for bit, reported norm and coefficient included, and the new threshold reaches the replays."""
    if "eager" not in _CLIPPED:
        _CLIPPED["eager"] = _clipped_run(pkg, dev, "eager")
    ref, got = _CLIPPED["eager"], _clipped_run(pkg, dev, mode)
    _assert_same(ref, got, mode)
    for k, (u, v) in enumerate(zip(ref, got)):
        assert same_bits(u["norm"], v["norm"]) and same_bits(u["coef"], v["coef"]), (mode, k)
        assert u["coef"] < 1.0
    base = _first_norm(pkg, dev)                                # the halved threshold took effect at replay 3, not before
    assert same_bits(got[2]["coef"], R.coef_f32(got[2]["norm"], 0.5 * base))
    assert same_bits(got[3]["coef"], R.coef_f32(got[3]["norm"], 0.25 * base))
    assert got[3]["coef"] != R.coef_f32(got[3]["norm"], 0.5 * base)


def test_bf16_communication_captured_equals_eager(pkg, dev):
    """(c) the bf16-communication form, whose norm reads the bf16 buffer the weight-gradient epilogue wrote: captured against eager"""
    ref, got = _clipped_run(pkg, dev, "dp_bf16_eager"), _clipped_run(pkg, dev, "dp_bf16")
    _assert_same(ref, got, "dp_bf16")
    for u, v in zip(ref, got):
        assert same_bits(u["norm"], v["norm"]) and same_bits(u["coef"], v["coef"]) and u["coef"] < 1.0


def test_switching_on_after_construction(pkg, dev):
    """an eager data-parallel TrainStep built without clipping follows set_max_grad_norm: the step reads the optimizer's setting when
    it launches, so the norm runs in front of the held-back AdamW launches -- same bits as a step built with clipping"""
    xd, yd = _data(dev)
    out = []
    for late in (False, True):
        m, flat, opt, crit = _build(pkg, dev, None if late else float("inf"))
        step = pkg.TrainStep(m, crit, opt, xd, yd, warmup=1, **_step_kwargs("dp_eager"))
        assert step.clip == (not late)
        if late:
            opt.set_max_grad_norm(float("inf"))
        opt.set_max_grad_norm(0.5)
        assert step.clip and "clipped by global norm" in step.launch
        step.run()
        out.append(_snap(flat, opt, step))
        flat["state"].clear()
        del step, opt, m, flat
    _assert_same([out[0], out[0]], [out[1], out[1]], "late switch")
    assert same_bits(out[0]["norm"], out[1]["norm"]) and same_bits(out[0]["coef"], out[1]["coef"]) and out[1]["coef"] < 1.0


def test_refusals(pkg, dev):
    """(d) the fused update cannot be clipped: TrainStep raises at construction, begin_fused_step raises; set_max_grad_norm during
    capture raises"""
    xd, yd = _data(dev)
    m, flat, opt, crit = _build(pkg, dev, 12.0)
    with pytest.raises(ValueError, match="fuse_update cannot be combined with gradient clipping"):
        pkg.TrainStep(m, crit, opt, xd, yd, fuse_update=True)
    with pytest.raises(RuntimeError, match="no global gradient norm exists"):
        opt.begin_fused_step(tuple(True for _ in flat["params"]))
    opt2 = pkg.AdamW([torch.nn.Parameter(g(8).to(dev))])
    with pytest.raises(ValueError, match="fuse_update cannot be combined with gradient clipping"):
        pkg.TrainStep(m, crit, opt2, xd, yd, fuse_update=True, max_grad_norm=3.0)
    assert opt2.max_grad_norm is None
    side = torch.cuda.Stream()
    buf = torch.zeros(8, device=dev)
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="while a hipGraph is being captured"):
        with torch.cuda.graph(graph, stream=side):
            buf.add_(1.0)
            opt.set_max_grad_norm(5.0)
    torch.cuda.synchronize()
    assert opt.max_grad_norm == 12.0
    flat["state"].clear()


def test_per_tensor_optimizer_path(pkg, dev):
    """AdamW(max_grad_norm=) without arenas, two param groups, one non-contiguous gradient: the norm is global over the groups and the
    update equals an unclipped optimizer on gradients scaled by the reported coefficient"""
    shapes = [(33,), (5, 7), (4099,)]
    grads = [g(*s, seed=20 + i, scale=0.5).to(dev) for i, s in enumerate(shapes)]
    grads[1] = g(7, 5, seed=21, scale=0.5).to(dev).t()
    assert not grads[1].is_contiguous()

    def make(max_norm):
        ps = [torch.nn.Parameter(g(*s, seed=i, scale=0.05).to(dev)) for i, s in enumerate(shapes)]
        return ps, pkg.AdamW([dict(params=ps[:2]), dict(params=ps[2:], lr=2e-3)], lr=LR, weight_decay=WD, max_grad_norm=max_norm)

    pa, a = make(1.0)
    for p, gr in zip(pa, grads):
        p.grad = gr.clone() if gr.is_contiguous() else gr
    a.step()
    norm, coef = float(a.grad_norm()), float(a.clip_coef())
    assert R.ulp_diff(norm, R.norm_f32([gr.cpu().numpy() for gr in grads])) <= 1
    assert coef < 1.0 and same_bits(coef, R.coef_f32(norm, 1.0))
    pb, b = make(None)
    for p, gr in zip(pb, grads):
        p.grad = gr.contiguous() * coef
    b.step()
    torch.cuda.synchronize()
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
    assert a.nonfinite_steps() == 0


def _free_case(dev, seed):
    shapes = [(1,), (3, 5), (4097,), (2, 3, 4, 5, 7)]
    params = [torch.nn.Parameter(torch.zeros(*s, device=dev)) for s in shapes] + [torch.nn.Parameter(torch.zeros(9, device=dev))]
    grads = [g(*s, seed=seed + i, scale=3.0).to(dev) for i, s in enumerate(shapes)]
    grads[1] = g(5, 3, seed=seed + 1, scale=3.0).to(dev).t()       # non-contiguous
    for p, gr in zip(params, grads):
        p.grad = gr.clone() if gr.is_contiguous() else gr.clone().t().contiguous().t()
    assert not params[1].grad.is_contiguous() and params[4].grad is None
    return params, grads


@pytest.mark.parametrize("max_norm", [1.0, 1e4, float("inf")])
def test_free_function_on_plain_tensors(pkg, dev, max_norm):
    """(e) clip_grad_norm_ on non-arena tensors, shapes (1,), (3, 5) non-contiguous, (4097,), (2, 3, 4, 5, 7), one parameter without
    a gradient: the norm within 1 ulp of float64, the gradients = g * coef bit for bit with that run's coefficient, and within 5e-7
    relative of the float64-derived product (a coefficient within 2 ulp plus one rounding of the product)."""
    params, grads = _free_case(dev, 50)
    row = pkg.grad_clip.clip_grad_norm_row_(params, max_norm)
    norm, coef = row[0].item(), row[1].item()
    host = [gr.cpu().numpy() for gr in grads]
    want = R.norm_f32(host)
    assert R.ulp_diff(norm, want) <= 1
    assert same_bits(coef, R.coef_f32(norm, max_norm)) and (coef < 1.0) == (max_norm == 1.0)
    s64 = np.sqrt(R.sumsq64(host))
    c64 = min(1.0, max_norm / (s64 + 1e-6))
    for p, gr, h in zip(params, grads, host):
        assert torch.equal(p.grad, gr * row[1])
        assert p.grad.stride() == gr.stride()
        exact = h.astype(np.float64) * c64
        assert np.all(np.abs(p.grad.cpu().numpy().astype(np.float64) - exact) <= 5e-7 * np.abs(exact))
    # the public function: torch's name and return value, the same bits
    params2, _ = _free_case(dev, 50)
    total = pkg.clip_grad_norm_(params2, max_norm)
    assert total.dim() == 0 and total.is_cuda and same_bits(total.item(), norm)
    for p, q in zip(params, params2[:4]):
        assert torch.equal(p.grad, q.grad)
    ref, _ = _free_case(dev, 50)
    tn = torch.nn.utils.clip_grad_norm_(ref, max_norm)
    assert abs(tn.item() - norm) <= 1e-6 * norm


def test_free_function_nonfinite_and_arena(pkg, dev):
    """error_if_nonfinite=True raises before anything is scaled; on a model's arena gradients the table path is taken and equals
    the float64 reference over the slices that have a gradient"""
    params, grads = _free_case(dev, 60)
    params[2].grad[5] = float("inf")
    keep = [p.grad.clone() for p in params[:4]]
    with pytest.raises(RuntimeError, match="non-finite"):
        pkg.clip_grad_norm_(params, 1.0, error_if_nonfinite=True)
    for p, k in zip(params, keep):
        assert torch.equal(p.grad, k)
    assert pkg.clip_grad_norm_(params, 1.0).item() == float("inf")
    assert float(params[3].grad.abs().max()) == 0.0                # coef = 0, as in torch

    xd, yd = _data(dev)
    m, flat, opt, crit = _build(pkg, dev, None)
    crit(m(xd), yd).backward()
    pattern = [p.grad is not None for p in flat["params"]]
    before = flat["grad"].clone()
    host = before.cpu().numpy()
    want = R.norm_f32([host[o:o + p.numel()] for p, o, has in zip(flat["params"], flat["offsets"], pattern) if has])
    assert pkg.grad_clip._arena_of([p for p in flat["params"] if p.grad is not None]) is not None
    row = pkg.grad_clip.clip_grad_norm_row_(m.parameters(), 0.5 * float(want))
    assert R.ulp_diff(row[0].item(), want) <= 1 and row[1].item() < 0.51
    for p, o, has in zip(flat["params"], flat["offsets"], pattern):
        sl = slice(o, o + p.numel())
        assert torch.equal(flat["grad"][sl], before[sl] * row[1] if has else before[sl])
    # the range table lives with the arena it describes, not in a process-wide cache keyed by an address the allocator can hand out again
    assert not hasattr(pkg.grad_clip, "_TABLES") and list(flat["_clip_tables"]) == [tuple(pattern)]
    table = flat["_clip_tables"][tuple(pattern)][0]
    opt.zero_grad(set_to_none=True)
    flat["state"].clear()
    del m, opt

    # a second model in the same process with another arena layout (4 classes: the last range is longer) builds its own table
    from oracle.unetr_oracle import synthetic_volume
    x4, y4 = synthetic_volume(2, 1, 32, 4, seed=41)
    torch.manual_seed(11)
    m2 = pkg.UNETRLogits(**dict(C1, out_channels=4)).to(dev)
    m2.precision = "bf16"
    flat2 = m2.use_flat_buffers()
    assert flat2["total"] != flat["total"] and len(flat2["params"]) == len(flat["params"])
    pkg.DiceCELoss(to_onehot_y=True, softmax=True)(m2(x4.to(dev)), y4.to(dev)).backward()
    pattern2 = [p.grad is not None for p in flat2["params"]]
    assert pattern2 == pattern                                    # the same key under the retired cache
    host = flat2["grad"].cpu().numpy()
    want = R.norm_f32([host[o:o + p.numel()] for p, o, has in zip(flat2["params"], flat2["offsets"], pattern2) if has])
    row = pkg.grad_clip.clip_grad_norm_row_(m2.parameters(), float("inf"))
    assert R.ulp_diff(row[0].item(), want) <= 1
    table2 = flat2["_clip_tables"][tuple(pattern2)][0]
    assert table2 is not table and not torch.equal(table2, table)
    for p in m2.parameters():
        p.grad = None
    flat2["state"].clear()
