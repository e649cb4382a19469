"""Device-resident AdamW hyper-parameters: the row {lr, weight_decay, t, reserved} that every optimizer kernel reads when it RUNS.

Kernel level (bitwise): the row forms against the by-value forms with the same float lr / weight_decay (unetr_adamw_hyper, and
arena.hyper in unetr_adamw_ranges / unetr_gemm_bf16_grouped_wgrad_adamw[_t]); the in-graph schedule on the step-counter launch
(unetr_counter_add_lr) against the host formula.  Model level (C1 geometry: 32^3, hidden 128, mlp 512, 4 heads): a host
lr_scheduler under hipGraph replay, the in-graph schedule, the capture rules, and checkpoint / resume in torch.optim.AdamW's schema."""
import ctypes
import struct
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

C1 = dict(in_channels=1, out_channels=2, img_size=(32, 32, 32), feature_size=16, hidden_size=128, mlp_dim=512,
          num_heads=4, pos_embed="perceptron", norm_name="instance", res_block=True)
LR, WD, B1, B2, EPS = 1e-3, 1e-2, 0.9, 0.999, 1e-8


def f32(x):
    return struct.unpack("f", struct.pack("f", float(x)))[0]


def g(*shape, seed=0, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=gen) * scale


# ---------------------------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("shadows", ["none", "bf16", "bf16+words"])
@pytest.mark.parametrize("g_bf16", [False, True])
def test_adamw_hyper_equals_by_value(pkg, dev, g_bf16, shadows):
    """unetr_adamw_hyper = unetr_adamw_reduced (and unetr_adamw where that applies) with the same lr / weight_decay, bit for bit:
    n = 4099 (more than one 4096-element block, a ragged tail of 3), fp32 and bf16 gradients with gscale = 0.5, with and without
    the bf16 shadow and the bf16x3 word shadow, step counts 1 and 3 on the same state."""
    capi = pkg._capi
    st = torch.cuda.current_stream().cuda_stream
    n = 4099
    p0 = g(n, seed=1, scale=0.05).to(dev)
    grads = [g(n, seed=2 + i, scale=0.01).to(dev) for i in range(2)]
    if g_bf16:
        grads = [x.bfloat16() for x in grads]
    # row 1 of a two-row table: lr / weight_decay are read from THIS row (row 0 holds other values)
    table = torch.tensor([[0.5, 0.5, 0.0, 0.0], [LR, WD, 0.0, 0.0]], dtype=torch.float32, device=dev)

    def run(form, gscale):
        p, m, v = p0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        sh = torch.zeros(n, device=dev, dtype=torch.bfloat16) if shadows != "none" else None
        wo = torch.zeros(n, device=dev, dtype=torch.int32) if shadows == "bf16+words" else None
        for grad, count in zip(grads, (1.0, 3.0)):
            step = torch.tensor([count], dtype=torch.float32, device=dev)
            shp, wop = (sh.data_ptr() if sh is not None else None), (wo.data_ptr() if wo is not None else None)
            if form == "hyper":
                capi.call("unetr_adamw_hyper", p.data_ptr(), grad.data_ptr(), int(g_bf16), gscale, m.data_ptr(), v.data_ptr(), n,
                          table.data_ptr() + 16, B1, B2, EPS, step.data_ptr(), shp, wop, st)
            elif form == "reduced":
                capi.call("unetr_adamw_reduced", p.data_ptr(), grad.data_ptr(), int(g_bf16), gscale, m.data_ptr(), v.data_ptr(), n,
                          LR, B1, B2, EPS, WD, step.data_ptr(), shp, wop, st)
            else:
                capi.call("unetr_adamw", p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, LR, B1, B2, EPS, WD,
                          step.data_ptr(), shp, st)
        torch.cuda.synchronize()
        return [t for t in (p, m, v, sh, wo) if t is not None]

    ref, new = run("reduced", 0.5), run("hyper", 0.5)
    assert len(ref) == len(new) == 3 + (shadows != "none") + (shadows == "bf16+words")
    for a, b in zip(ref, new):
        assert torch.equal(a, b)
    assert (ref[0] != p0).float().mean() > 0.99                  # every parameter moved
    if not g_bf16 and shadows != "bf16+words":                   # the per-tensor entry point: fp32 gradients, gscale 1, no word shadow
        for a, b in zip(run("plain", 1.0), run("hyper", 1.0)):
            assert torch.equal(a, b)


@pytest.mark.parametrize("twin", [False, True])
def test_arena_hyper_equals_by_value(pkg, dev, twin):
    """arena.hyper set against the by-value fields: unetr_gemm_bf16_grouped_wgrad_adamw (twin: its _t form, which also writes the
    transposed bf16 shadow) and unetr_adamw_ranges over the parameters between the weight matrices, on the problem shapes of
    test_grouped_wgrad_fused_epilogues (ragged tiles, a ragged token count), two steps, per-parameter step counts.  With the row
    set the by-value fields hold OTHER values: the row is what the kernels read."""
    capi = pkg._capi
    st = torch.cuda.current_stream().cuda_stream
    shapes = [(432, 768, 256), (216, 200, 136), (64, 8, 8), (432, 128, 384)]
    sizes, is_w = [40], [False]
    for k, (_, N, K) in enumerate(shapes):
        sizes += [N * K, (48, 8, 0, 24)[k]]
        is_w += [True, False]
    sizes, is_w = zip(*[(n, w) for n, w in zip(sizes, is_w) if n])
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += n
    nparam = len(sizes)
    widx = [i for i, w in enumerate(is_w) if w]
    p0 = g(total, seed=5, scale=0.05).to(dev)
    grads_other = g(total, seed=6, scale=0.01).to(dev)
    ops = [(g(M, N, seed=30 + i).bfloat16().to(dev), g(M, K, seed=40 + i).bfloat16().to(dev)) for i, (M, N, K) in enumerate(shapes)]
    row = torch.tensor([LR, WD, 0.0, 0.0], dtype=torch.float32, device=dev)

    def run(use_row):
        p, m, v = p0.clone(), torch.zeros(total, device=dev), torch.zeros(total, device=dev)
        shadow = torch.zeros(total, device=dev, dtype=torch.bfloat16)
        tw = torch.zeros(total, device=dev, dtype=torch.bfloat16)
        steps = torch.zeros(nparam, device=dev)
        steps[1] = 3.0
        for it in range(2):
            grad = grads_other.clone() * (it + 1)
            steps += 1.0
            arr = (capi.GroupedProblem * len(shapes))()
            for i, ((dy, x), (M, N, K)) in enumerate(zip(ops, shapes)):
                arr[i].dy, arr[i].x, arr[i].dw = dy.data_ptr(), x.data_ptr(), grad.data_ptr() + 4 * offs[widx[i]]
                arr[i].M, arr[i].N, arr[i].K = M, N, K
            lr, wd = (0.25, 0.5) if use_row else (LR, WD)
            arena = capi.AdamWArena(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), shadow.data_ptr(), steps.data_ptr(), total,
                                    lr, B1, B2, EPS, wd, None, row.data_ptr() if use_row else None)
            sidx = (ctypes.c_int * len(shapes))(*widx)
            if twin:
                capi.call("unetr_gemm_bf16_grouped_wgrad_adamw_t", arr, len(shapes), ctypes.byref(arena), sidx, tw.data_ptr(), st)
            else:
                capi.call("unetr_gemm_bf16_grouped_wgrad_adamw", arr, len(shapes), ctypes.byref(arena), sidx, st)
            rows, blocks = [], 0
            for i in range(nparam):
                if not is_w[i]:
                    rows.append((offs[i], offs[i] + sizes[i], i, blocks))
                    blocks += (sizes[i] + 4095) // 4096
            table = torch.tensor(rows, dtype=torch.int64, device=dev)
            capi.call("unetr_adamw_ranges", ctypes.byref(arena), table.data_ptr(), len(rows), blocks, st)
        torch.cuda.synchronize()
        return p, m, v, shadow, tw

    ref, new = run(False), run(True)
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq", "shadow", "twin"), ref, new):
        assert torch.equal(a, b), name
    assert (ref[0] != p0).float().mean() > 0.99
    assert bool((ref[4] != 0).any()) == twin


SCHEDULE_CASES = [
    ("constant", dict(), {0: "base", 7: "base"}),
    ("constant", dict(min_lr=5e-3), {0: "min", 3: "min"}),
    ("warmup_cosine", dict(warmup=2, total=6), {2: "base", 6: "min", 7: "min"}),
    ("warmup_cosine", dict(warmup=2, total=6, min_lr=1e-5), {0: "min", 2: "base", 6: "min", 7: "min"}),
    ("poly", dict(total=4, power=2.0), {0: "base", 4: "min", 7: "min"}),
]


@pytest.mark.parametrize("kind,kw,exact", SCHEDULE_CASES)
def test_counter_add_lr(pkg, dev, kind, kw, exact):
    """8 consecutive launches of unetr_counter_add_lr: the counters are those of unetr_counter_add, t counts up, lr is
    schedule_lr(s) to 1e-6 relative (one float32 rounding, 6e-8, plus a double-precision cos / pow ulp) and EXACTLY base_lr /
    min_lr at the points where the formula gives f = 1 / f = 0; weight_decay and the neighbouring row are not touched."""
    capi = pkg._capi
    st = torch.cuda.current_stream().cuda_stream
    n = 300                                                      # two 256-thread blocks, a ragged second one
    inc = (g(n, seed=3) > 0).float().to(dev)
    y, y_ref = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    table = torch.tensor([[7.0, 8.0, 9.0, 10.0], [123.0, WD, 0.0, 0.0]], dtype=torch.float32, device=dev)
    desc = dict(kind=kind, base_lr=LR, warmup=kw.get("warmup", 0), total=kw.get("total", 0), power=kw.get("power", 0.9),
                min_lr=kw.get("min_lr", 0.0))
    sc = capi.LrSchedule(pkg.optim.SCHEDULES[kind], desc["base_lr"], desc["min_lr"], desc["warmup"], desc["total"], desc["power"])
    seen = []
    for s in range(8):
        capi.call("unetr_counter_add_lr", y.data_ptr(), inc.data_ptr(), n, table.data_ptr() + 16, ctypes.byref(sc), st)
        capi.call("unetr_counter_add", y_ref.data_ptr(), inc.data_ptr(), n, st)
        seen.append(table.cpu().clone())
    assert torch.equal(y, y_ref) and torch.equal(y, inc * 8)
    for s, tab in enumerate(seen):
        assert tab[0].tolist() == [7.0, 8.0, 9.0, 10.0]
        lr, wd, t, _ = tab[1].tolist()
        want = pkg.optim.schedule_lr(desc, s)
        print(f"{kind} {kw} s={s}: device lr {lr!r} host {want!r}")
        assert t == s + 1 and wd == f32(WD)
        assert abs(lr - want) <= 1e-6 * abs(want)
        if s in exact:
            assert lr == (f32(LR) if exact[s] == "base" else f32(desc["min_lr"]))
    # no schedule (NULL): the host's lr stays, t still counts
    capi.call("unetr_counter_add_lr", y.data_ptr(), inc.data_ptr(), n, table.data_ptr() + 16, None, st)
    assert torch.equal(y, inc * 9)
    assert table[1].tolist()[0] == seen[-1][1, 0].item() and table[1, 2].item() == 9.0


# ----------------------------------------------------------------------------------------------------------------- model level
def _data(dev):
    from oracle.unetr_oracle import synthetic_volume
    x, y = synthetic_volume(2, 1, 32, 2, seed=41)
    return x.to(dev), y.to(dev)


def _build(pkg, dev, *, lr=LR, wd=1e-5):
    torch.manual_seed(11)
    m = pkg.UNETRLogits(**C1).to(dev)
    m.precision = "bf16"
    flat = m.use_flat_buffers()
    opt = pkg.AdamW(m.parameters(), lr=lr, weight_decay=wd, flat=flat)
    return m, flat, opt, pkg.DiceCELoss(to_onehot_y=True, softmax=True)


def _snap(flat, opt, step):
    torch.cuda.synchronize()
    return (flat["param"].clone(), opt._flat_state[0].clone(), opt._flat_state[1].clone(), flat["shadow"].clone(), float(step.loss.detach()))


def _host_scheduled_run(pkg, dev, mode, wd_change):
    """4 steps with torch.optim.lr_scheduler.LambdaLR stepped after each; the state after every step"""
    xd, yd = _data(dev)
    m, flat, opt, crit = _build(pkg, dev)
    step = pkg.TrainStep(m, crit, opt, xd, yd, use_graph=mode != "eager", fuse_update=mode == "fused", overlap_update=mode == "overlap")
    if mode == "fused":
        assert step.fuse and "epilogue" in step.launch
    if mode == "overlap":
        assert step.one_graph and len(step.graphs) == 1
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (a replay never calls optimizer.step() in Python: the scheduler's order check warns)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: 0.5 ** k)
        out = []
        for k in range(4):
            step.run()
            out.append(_snap(flat, opt, step))
            sched.step()
            if wd_change:
                opt.param_groups[0]["weight_decay"] = 1e-2 * (k + 1)
    assert opt.param_groups[0]["lr"] == LR * 0.5 ** 4
    flat["state"].clear()
    return out


_EAGER = {}


@pytest.mark.parametrize("mode,wd_change", [("fused", False), ("overlap", False), ("fused", True)])
def test_host_scheduler_under_replay(pkg, dev, mode, wd_change):
    """A host lr_scheduler (and a weight_decay change between steps) must reach a CAPTURED step: after every one of 4 replays the
    masters, both moments, the bf16 shadow and the loss equal, bit for bit, those of the eager TrainStep on an identically seeded
    model with the same scheduler.  fused: one graph, AdamW of the ViT weights in the weight-gradient epilogue + the range launch;
    overlap: the reduced launch form, one graph with the side-stream branch.  (With lr baked into the graph as a kernel argument
    the replays keep the capture-time rate and the second step already differs.)"""
    if wd_change not in _EAGER:
        _EAGER[wd_change] = _host_scheduled_run(pkg, dev, "eager", wd_change)
    ref, got = _EAGER[wd_change], _host_scheduled_run(pkg, dev, mode, wd_change)
    for k, (a, b) in enumerate(zip(ref, got)):
        for name, u, v in zip(("param", "exp_avg", "exp_avg_sq", "shadow"), a, b):
            assert torch.equal(u, v), (k, name)
        assert a[4] == b[4], (k, "loss")
    assert not torch.equal(ref[0][0], ref[3][0])


def test_in_graph_schedule(pkg, dev):
    """set_schedule("warmup_cosine", warmup=2, total=5) before capture, 6 replays: the device's lr after each replay follows
    schedule_lr (1e-6 relative: one float32 rounding + a double cos ulp), and the parameters equal, bit for bit, those of an eager
    run whose group["lr"] is set on the host to the values the device reported.  (The eager warm-up steps before capture are steps
    0 and 1 of the schedule: f = 0 and 1/2, exact in any arithmetic.)  set_schedule on the captured optimizer raises."""
    xd, yd = _data(dev)
    m, flat, opt, crit = _build(pkg, dev)
    opt.set_schedule("warmup_cosine", warmup=2, total=5)
    step = pkg.TrainStep(m, crit, opt, xd, yd, use_graph=True, fuse_update=True)
    s0 = step.eager_steps
    assert s0 == 2 and len(step.graphs) == 1
    reported = []
    for k in range(6):
        step.run()
        reported.append(opt.current_lr())
    for k, lr in enumerate(reported):
        want = opt.schedule_lr(s0 + k)
        print(f"s={s0 + k}: device lr {lr!r} host {want!r}")
        assert abs(lr - want) <= 1e-6 * abs(want)
    assert reported[0] == f32(LR) and reported[3:] == [0.0, 0.0, 0.0]            # s = 2: f = 1; s >= 5: f = 0
    got = _snap(flat, opt, step)
    assert int(opt._hyper[0, 2]) == 8
    with pytest.raises(RuntimeError, match="before TrainStep captures"):
        opt.set_schedule("poly", total=10)
    flat["state"].clear()

    lrs = [opt.schedule_lr(0), opt.schedule_lr(1)] + reported
    m, flat, opt, crit = _build(pkg, dev, lr=lrs[0])
    step = pkg.TrainStep(m, crit, opt, xd, yd, use_graph=False, warmup=1)
    for lr in lrs[1:]:
        opt.param_groups[0]["lr"] = lr
        step.run()
    ref = _snap(flat, opt, step)
    for name, u, v in zip(("param", "exp_avg", "exp_avg_sq", "shadow"), ref, got):
        assert torch.equal(u, v), name
    assert ref[4] == got[4]
    flat["state"].clear()


def test_sync_hyper_during_capture_raises(pkg, dev):
    """An upload recorded into a graph would reset the rate on every replay: sync_hyper does nothing while the stream is capturing,
    and raises when a change is pending there."""
    p = torch.nn.Parameter(g(37, seed=1).to(dev))
    opt = pkg.AdamW([p], lr=LR, weight_decay=WD)
    p.grad = g(37, seed=2).to(dev)
    opt.step()
    torch.cuda.synchronize()
    assert opt._hyper[0].tolist() == [f32(LR), f32(WD), 1.0, 0.0]
    side = torch.cuda.Stream()
    buf = torch.zeros(8, device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        buf.add_(1.0)
        opt.sync_hyper()                                        # nothing pending: no launch, no error
    opt.param_groups[0]["lr"] = 0.5
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="while a hipGraph is being captured"):
        with torch.cuda.graph(graph, stream=side):
            buf.add_(1.0)
            opt.sync_hyper()
    torch.cuda.synchronize()
    assert opt._hyper[0, 0].item() == f32(LR)                   # nothing was written
    opt.sync_hyper()
    assert opt._hyper[0, 0].item() == 0.5


def test_resume_after_capture(pkg, dev):
    """Checkpoint / resume on the fast path.  Run A: captured fused step with a schedule, reset to the initial state AFTER capture
    (load_state_dict of the initial dicts: in place, the graph stays valid), 2 steps, save model and optimizer state_dict(), 2
    more steps.  Run B: fresh model, optimizer and TrainStep, both dicts loaded after capture, 2 steps.  B must equal A's 4
    uninterrupted steps bit for bit (masters, moments, loss).  The same dict loads into torch.optim.AdamW with step == 2."""
    xd, yd = _data(dev)

    def start():
        m, flat, opt, crit = _build(pkg, dev)
        opt.set_schedule("warmup_cosine", warmup=1, total=6, min_lr=1e-5)
        init = ({k: v.clone() for k, v in m.state_dict().items()}, opt.state_dict())
        assert init[1]["state"] == {} and init[1]["param_groups"][0]["t"] == 0
        step = pkg.TrainStep(m, crit, opt, xd, yd, use_graph=True, fuse_update=True)
        assert len(opt.state) == 0                              # flat mode: the moments live in the arenas, self.state stays empty
        return m, flat, opt, step, init

    def load(m, opt, model_sd, opt_sd):
        m.load_state_dict(model_sd)
        opt.load_state_dict(opt_sd)
        pkg.refresh_derived_weights(m)                          # the captured step reads the optimizer-maintained copies as they are

    m, flat, opt, step, init = start()
    ptrs = (opt._flat_state[0].data_ptr(), opt._steps[0].data_ptr(), opt._hyper.data_ptr())
    load(m, opt, *init)
    assert ptrs == (opt._flat_state[0].data_ptr(), opt._steps[0].data_ptr(), opt._hyper.data_ptr())      # in place
    assert not opt._flat_state[0].any() and not opt._steps[0].any() and opt._hyper[0, 2].item() == 0.0
    step.run()
    step.run()
    torch.cuda.synchronize()
    saved = ({k: v.clone() for k, v in m.state_dict().items()}, opt.state_dict())
    assert saved[1]["param_groups"][0]["t"] == 2 and saved[1]["param_groups"][0]["schedule"]["kind"] == "warmup_cosine"
    assert len(opt.state) == 0
    stepped = [i for i, p in enumerate(flat["params"]) if i in saved[1]["state"]]
    assert 0 < len(stepped) < len(flat["params"])                # (MONAI's unused cls_token never steps: no entry, as in torch)
    assert all(float(saved[1]["state"][i]["step"]) == 2.0 for i in stepped)
    step.run()
    step.run()
    want = _snap(flat, opt, step)
    # the dict in torch's own optimizer over the same parameters
    topt = torch.optim.AdamW(m.parameters(), lr=LR)
    topt.load_state_dict(saved[1])
    for i in stepped:
        st = topt.state[flat["params"][i]]
        assert st["step"] == 2 and torch.equal(st["exp_avg"], saved[1]["state"][i]["exp_avg"])
    assert topt.param_groups[0]["weight_decay"] == 1e-5 and topt.param_groups[0]["decoupled_weight_decay"] is True
    flat["state"].clear()
    del step, opt, m, flat, topt

    m, flat, opt, step, _ = start()
    load(m, opt, *saved)
    assert opt._host_steps[stepped[0]] == 2
    step.run()
    step.run()
    got = _snap(flat, opt, step)
    for name, u, v in zip(("param", "exp_avg", "exp_avg_sq", "shadow"), want, got):
        assert torch.equal(u, v), name
    assert want[4] == got[4]
    assert opt.state_dict()["param_groups"][0]["t"] == 4
    flat["state"].clear()


def test_per_tensor_state_dict_round_trip(pkg, dev):
    """Per-tensor mode (no flat=): state[i] carries "step"; the dict round-trips through this optimizer (bit-identical third step)
    and through torch.optim.AdamW in both directions."""
    shapes = [(33,), (5, 7), (4099,)]
    grads = [[g(*s, seed=10 * k + i, scale=0.01).to(dev) for i, s in enumerate(shapes)] for k in range(3)]

    def params():
        return [torch.nn.Parameter(g(*s, seed=i, scale=0.05).to(dev)) for i, s in enumerate(shapes)]

    def take(opt, ps, k, skip_last=False):
        for p, gr in zip(ps, grads[k]):
            p.grad = gr.clone()
        if skip_last:
            ps[-1].grad = None
        opt.step()

    pa = params()
    a = pkg.AdamW(pa, lr=LR, weight_decay=WD)
    take(a, pa, 0, skip_last=True)                               # the last parameter steps once, the others twice
    take(a, pa, 1)
    sd = a.state_dict()
    assert [float(sd["state"][i]["step"]) for i in range(3)] == [2.0, 2.0, 1.0] and sd["param_groups"][0]["t"] == 2
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    b = pkg.AdamW(pb, lr=5.0, weight_decay=0.0)
    b.load_state_dict(sd)
    assert b.param_groups[0]["lr"] == LR and b.param_groups[0]["weight_decay"] == WD
    pt = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    t = torch.optim.AdamW(pt, lr=5.0)
    t.load_state_dict(sd)
    assert [float(t.state[p]["step"]) for p in pt] == [2.0, 2.0, 1.0]
    take(a, pa, 2)
    take(b, pb, 2)
    take(t, pt, 2)
    torch.cuda.synchronize()
    for x, y, z in zip(pa, pb, pt):
        assert torch.equal(x, y)
        assert torch.allclose(x, z, rtol=1e-5, atol=1e-7)        # torch's eager AdamW: the same update in another operation order
    # and back: torch's dict into this optimizer
    pc = [torch.nn.Parameter(p.detach().clone()) for p in pt]
    c = pkg.AdamW(pc, lr=5.0)
    c.load_state_dict(t.state_dict())
    sc = c.state_dict()
    assert [float(sc["state"][i]["step"]) for i in range(3)] == [3.0, 3.0, 2.0] and sc["param_groups"][0]["t"] == 3
    for i, p in enumerate(pt):
        assert torch.equal(sc["state"][i]["exp_avg"], t.state[p]["exp_avg"]) and torch.equal(sc["state"][i]["exp_avg_sq"], t.state[p]["exp_avg_sq"])
