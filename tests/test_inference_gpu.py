"""SlidingWindowInferer and Gaussian blending on the GPU: against the CPU restatement driving the oracle model, against the
per-window function bit for bit (captured and eager, both blending modes, fp32 and bf16), the three new kernels through the C
ABI, the fused post-processing forms, and weight freshness of the captured forward next to a live TrainStep."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from inference_ref import ref_importance_map, ref_sliding_window
from test_model_gpu import C1, _pair
from util import relerr

pytestmark = pytest.mark.gpu

ROI = (32, 32, 32)
# (volume, batch, overlap, sw_batch_size): 8 windows per item | 8 | interval 6: 64 windows | 8 | 6 = one full row + a tail of 2 |
# 2 = tail only | smaller than the window: the padding path | 8 in rows of 3: tail of 2
CASES = [((48, 48, 48), 2, 0.25, 4), ((40, 40, 40), 1, 0.5, 4), ((48, 48, 48), 1, 0.8, 4), ((40, 48, 56), 1, 0.25, 4),
         ((32, 48, 80), 1, 0.25, 4), ((32, 32, 56), 1, 0.25, 4), ((24, 24, 24), 2, 0.25, 4), ((48, 48, 48), 1, 0.25, 3)]


def _volume(size, batch, channels=1, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(batch, channels, *size, generator=g)


def _hip_model(pkg, dev, cfg, seed=3, cls=None):
    torch.manual_seed(seed)
    return (cls or pkg.UNETR)(**cfg).to(dev)


# ---------------------------------------------------------------------------------------------- 1. against the restatement
def test_gaussian_blending_matches_reference_restatement(pkg, dev):
    ref, hip = _pair(pkg, dev, C1, seed=4, ref_dtype=torch.float32)
    hip.precision = "fp32"
    ref_pred = lambda w: ref(w)[1]
    runs = [(c, 0.125) for c in CASES] + [(CASES[3], 0.05)]
    inferers = {}
    for k, ((size, batch, overlap, n), sigma) in enumerate(runs):
        x = _volume(size, batch, seed=k)
        imp = ref_importance_map(ROI, "gaussian", sigma)
        with torch.no_grad():
            out_r = ref_sliding_window(x, ROI, n, ref_pred, overlap=overlap, importance=imp)
        out_f = pkg.sliding_window_inference(x.to(dev), ROI, n, hip, overlap=overlap, mode="gaussian", sigma_scale=sigma)
        key = (n, overlap, sigma)
        if key not in inferers:
            inferers[key] = pkg.SlidingWindowInferer(ROI, n, overlap=overlap, mode="gaussian", sigma_scale=sigma)
        out_i = inferers[key](x.to(dev), hip)
        assert out_f.shape == out_i.shape == out_r.shape == (batch, 2, *size)
        e_f, e_i = relerr(out_f, out_r), relerr(out_i, out_r)
        print(f"gaussian {size} B={batch} overlap={overlap} n={n} sigma={sigma}: function {e_f:.3e}, inferer {e_i:.3e}")
        assert e_f < 1e-3 and e_i < 1e-3, (size, overlap, sigma)


# ---------------------------------------------------------------------------------------------- 2. inferer == function
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["constant", "gaussian"])
@pytest.mark.parametrize("use_graph", [True, False])
def test_inferer_equals_function_bit_for_bit(pkg, dev, use_graph, mode, precision):
    hip = _hip_model(pkg, dev, C1)
    hip.precision = precision
    inferers = {}
    sizes_seen = {}
    for k, (size, batch, overlap, n) in enumerate(CASES):
        x = _volume(size, batch, seed=10 + k).to(dev)
        inferer = inferers.get((n, overlap))
        if inferer is None:
            inferer = inferers[(n, overlap)] = pkg.SlidingWindowInferer(ROI, n, overlap=overlap, mode=mode, use_graph=use_graph)
        want = pkg.sliding_window_inference(x, ROI, n, hip, overlap=overlap, mode=mode)
        got = inferer(x, hip)
        assert got.shape == want.shape and torch.equal(got, want), (size, batch, overlap, n)
        assert torch.equal(inferer(x, hip), got), "a second call returns other bits"
        _, counts = pkg.inference.plan_window_table(batch, [max(v, 32) for v in size], ROI, overlap, n)
        sizes_seen.setdefault((n, overlap), set()).update(counts)
    for key, inferer in inferers.items():
        if use_graph:
            # one graph per distinct batch size (full rows, each tail size), never one per volume
            assert inferer.stats["captures"] == len(sizes_seen[key]) and inferer.stats["recaptures"] == 0, (key, inferer.stats)
            assert inferer.stats["replays"] > 0 and inferer.stats["eager_rows"] == 0
        else:
            assert inferer.stats["captures"] == 0 and inferer.stats["eager_rows"] > 0


def test_one_graph_serves_every_volume_size(pkg, dev):
    """volumes of six sizes at one overlap through ONE inferer: rows of 4, tails of 2 and of 1 -> three captures, not six"""
    hip = _hip_model(pkg, dev, C1)
    hip.precision = "bf16"
    inferer = pkg.SlidingWindowInferer(ROI, 4, overlap=0.25, mode="gaussian")
    seen, sizes = [], set()
    for k, size in enumerate([(48, 48, 48), (40, 48, 56), (32, 48, 80), (32, 32, 56), (24, 24, 24), (40, 40, 40)]):
        x = _volume(size, 1, seed=30 + k).to(dev)
        assert torch.equal(inferer(x, hip), pkg.sliding_window_inference(x, ROI, 4, hip, mode="gaussian")), size
        sizes.update(pkg.inference.plan_window_table(1, [max(v, 32) for v in size], ROI, 0.25, 4)[1])
        seen.append((inferer.stats["captures"], len(sizes)))
    assert sizes == {4, 2, 1}
    assert all(c == s for c, s in seen) and seen[0][0] == seen[1][0] == 1 and inferer.stats["captures"] == 3, seen
    assert inferer.stats["recaptures"] == 0


# ---------------------------------------------------------------------------------------------- 3. kernels through the C ABI
def _descriptor(pkg, dev, **kw):
    vol = pkg._capi.SwVolume()
    for k, v in kw.items():
        setattr(vol, k, v)
    return torch.frombuffer(bytearray(bytes(vol)), dtype=torch.uint8).to(dev)


def _table(pkg, dev, rows):
    """rows: lists of (b, z, y, x)"""
    t = torch.zeros(len(rows), pkg._capi.SW_ROW_INTS, dtype=torch.int32)
    for r, slots in enumerate(rows):
        t[r, 0] = len(slots)
        if slots:
            t[r, 4:4 + 4 * len(slots)] = torch.tensor(slots, dtype=torch.int32).flatten()
    return t.to(dev)


@pytest.mark.parametrize("in_size,roi,corners", [
    ((20, 22, 26), (32, 32, 32), [(0, 0, 0)]),                                              # hangs over every face
    ((40, 36, 50), (32, 32, 32), [(0, 0, 0), (8, 4, 18), (3, 1, 1), (5, 2, 3)]),            # unaligned x corners
    ((20, 40, 30), (32, 32, 32), [(0, 0, 0), (0, 8, 0), (0, 3, 0)]),                        # padded along z and x only
    ((9, 7, 13), (8, 6, 10), [(0, 0, 0), (1, 1, 3), (1, 0, 2)]),                            # window extent not a multiple of 4
])
def test_gather_batch_equals_pad_and_slice(pkg, dev, in_size, roi, corners):
    B, Cin, cval = 2, 3, -1.5
    x = _volume(in_size, B, channels=Cin, seed=50).to(dev)
    pads = [max(r - s, 0) for r, s in zip(roi, in_size)]
    lo = [p // 2 for p in pads]
    padded = F.pad(x, (lo[2], pads[2] - lo[2], lo[1], pads[1] - lo[1], lo[0], pads[0] - lo[0]), value=cval)
    D, H, W = padded.shape[2:]
    n = 4
    slots = [(k % B,) + c for k, c in enumerate(corners)]
    table = _table(pkg, dev, [slots])
    desc = _descriptor(pkg, dev, in_=x.data_ptr(), table=table.data_ptr(), B=B, Cin=Cin, C=1, Di=in_size[0], Hi=in_size[1],
                       Wi=in_size[2], D=D, H=H, W=W, pz=lo[0], py=lo[1], px=lo[2], cval=cval, rows=1, cursor=-1)
    dst = torch.full((n, Cin, *roi), 7.0, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    pkg._capi.call("unetr_sw_advance", desc.data_ptr(), s)
    pkg._capi.call("unetr_sw_gather_batch", desc.data_ptr(), dst.data_ptr(), n, Cin, *roi, s)
    torch.cuda.synchronize()
    for j, (b, z, y, xx) in enumerate(slots):
        assert torch.equal(dst[j], padded[b, :, z:z + roi[0], y:y + roi[1], xx:xx + roi[2]]), j
    assert bool((dst[len(slots):] == cval).all())              # inactive slots
    # a cursor past the table touches nothing
    dst.fill_(7.0)
    pkg._capi.call("unetr_sw_advance", desc.data_ptr(), s)
    pkg._capi.call("unetr_sw_gather_batch", desc.data_ptr(), dst.data_ptr(), n, Cin, *roi, s)
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all())


@pytest.mark.parametrize("size,overlap,n,roi,with_imp", [
    ((48, 48, 48), 0.8, 4, (32, 32, 32), True),          # heavy overlap inside every row
    ((48, 48, 48), 0.8, 16, (32, 32, 32), True),
    ((48, 48, 48), 0.8, 3, (32, 32, 32), True),          # 64 windows in rows of 3: the last row has inactive slots
    ((40, 42, 45), 0.5, 4, (32, 32, 32), True),          # rows of the volume not 16-byte aligned
    ((40, 42, 45), 0.5, 4, (32, 32, 32), False),         # importance = NULL
    ((20, 19, 23), 0.5, 5, (8, 6, 10), True),            # scalar variant
])
def test_accumulate_batch_equals_sequential_accumulate(pkg, dev, size, overlap, n, roi, with_imp):
    B, C = 2, 3
    D, H, W = size
    g = torch.Generator().manual_seed(77)
    imp = (torch.rand(*roi, generator=g) + 0.05).to(dev) if with_imp else None
    table_cpu, counts = pkg.inference.plan_window_table(B, size, roi, overlap, n)
    table = table_cpu.to(dev)
    out_a = torch.zeros(B, C, D, H, W, device=dev)
    cnt_a = torch.zeros(B, D, H, W, device=dev)
    out_b, cnt_b = torch.zeros_like(out_a), torch.zeros_like(cnt_a)
    desc = _descriptor(pkg, dev, out=out_a.data_ptr(), count=cnt_a.data_ptr(), table=table.data_ptr(), B=B, Cin=1, C=C,
                       Di=D, Hi=H, Wi=W, D=D, H=H, W=W, rows=len(counts), cursor=-1)
    s = torch.cuda.current_stream().cuda_stream
    ip = imp.data_ptr() if imp is not None else None
    segs = []
    for r, m in enumerate(counts):
        seg = torch.randn(n, C, *roi, generator=g).to(dev)
        segs.append(seg)
        pkg._capi.call("unetr_sw_advance", desc.data_ptr(), s)
        pkg._capi.call("unetr_sw_accumulate_batch", desc.data_ptr(), seg.data_ptr(), ip, n, C, *roi, s)
        for j in range(m):
            b, z, y, x = table_cpu[r, 4 + 4 * j:8 + 4 * j].tolist()
            pkg._capi.call("unetr_sw_accumulate", seg[j].data_ptr(), ip, out_b[b].data_ptr(), cnt_b[b].data_ptr(), C, *roi, D, H, W,
                           z, y, x, s)
    torch.cuda.synchronize()
    assert counts[-1] < n or len(counts) * n == sum(counts)
    assert torch.equal(cnt_a, cnt_b) and torch.equal(out_a, out_b)
    assert float(cnt_a.min()) > 0


@pytest.mark.parametrize("C,V", [(2, 4096), (14, 4099), (3, 1000)])
def test_finalize_post_forms(pkg, dev, C, V):
    B = 2
    g = torch.Generator().manual_seed(5)
    sums = torch.randn(B, C, V, generator=g)
    sums[:, :, ::7] = sums[:, :1, ::7]                     # exact ties across all channels
    if C > 2:
        sums[:, 2, 1::5] = sums[:, 1, 1::5]                # and between two channels
    cnt = torch.rand(B, V, generator=g) + 0.5
    sums, cnt = sums.to(dev), cnt.to(dev)
    s = torch.cuda.current_stream().cuda_stream
    want = sums.clone()
    pkg._capi.call("unetr_sw_finalize", want.data_ptr(), cnt.data_ptr(), B, C, V, s)
    got = sums.clone()
    pkg._capi.call("unetr_sw_finalize_post", got.data_ptr(), cnt.data_ptr(), None, B, C, V, 0, s)
    assert torch.equal(got, want)
    am = want.argmax(dim=1)
    got = sums.clone()
    pkg._capi.call("unetr_sw_finalize_post", got.data_ptr(), cnt.data_ptr(), None, B, C, V, 1, s)
    assert torch.equal(got, F.one_hot(am, C).movedim(-1, 1).float())
    got, ids = sums.clone(), torch.empty(B, V, device=dev)
    pkg._capi.call("unetr_sw_finalize_post", got.data_ptr(), cnt.data_ptr(), ids.data_ptr(), B, C, V, 2, s)
    assert torch.equal(ids, am.float())
    got = sums.clone()
    pkg._capi.call("unetr_sw_finalize_post", got.data_ptr(), cnt.data_ptr(), None, B, C, V, 3, s)
    assert torch.equal(got, (want >= 0).float())


# ---------------------------------------------------------------------------------------------- 4. post forms end to end
@pytest.mark.parametrize("classes", [2, 14])
def test_post_onehot_and_argmax(pkg, dev, classes):
    hip = _hip_model(pkg, dev, dict(C1, out_channels=classes))
    hip.precision = "fp32"
    inferer = pkg.SlidingWindowInferer(ROI, 4, overlap=0.5, mode="gaussian")
    x = _volume((40, 48, 44), 2, seed=60).to(dev)
    logits = inferer(x, hip)
    am = logits.argmax(dim=1)
    onehot = inferer(x, hip, post="onehot")
    assert onehot.shape == logits.shape and torch.equal(onehot, F.one_hot(am, classes).movedim(-1, 1).float())
    ids = inferer(x, hip, post="argmax")
    assert ids.shape == (2, 1, 40, 48, 44) and torch.equal(ids, am.unsqueeze(1).float())
    # DiceMetric fed the one-hot prediction = DiceMetric fusing argmax + one-hot over the logits
    y = torch.randint(0, classes, (2, 1, 40, 48, 44), generator=torch.Generator().manual_seed(1)).float().to(dev)
    m1, m2 = pkg.DiceMetric(), pkg.DiceMetric()
    m1(y_pred=onehot.contiguous(), y=F.one_hot(y.squeeze(1).long(), classes).movedim(-1, 1).float())
    m2(logits.contiguous(), y, from_logits=True)
    assert torch.equal(m1.aggregate(), m2.aggregate())


def test_post_argmax_takes_the_first_maximum_on_exact_ties(pkg, dev):
    """a predictor whose channels 1 and 2 are identical (and all four equal where the input is 0): blending keeps them
    identical, so every voxel is an exact tie"""
    pred = lambda w: torch.cat([w * 0.5, w, w, -w], 1)
    g = torch.Generator().manual_seed(2)
    x = torch.randint(-3, 4, (1, 1, 40, 40, 48), generator=g).float().to(dev)
    assert int((x == 0).sum()) > 1000
    for mode in ("constant", "gaussian"):
        inferer = pkg.SlidingWindowInferer(ROI, 4, overlap=0.5, mode=mode)
        logits = inferer(x, pred)
        assert torch.equal(logits[:, 1], logits[:, 2])
        am = logits.argmax(dim=1)
        assert set(am.unique().tolist()) == {0, 1, 3}          # never channel 2
        assert torch.equal(inferer(x, pred, post="argmax"), am.unsqueeze(1).float())
        assert torch.equal(inferer(x, pred, post="onehot"), F.one_hot(am, 4).movedim(-1, 1).float())
        assert inferer.stats["captures"] == 0


def test_post_sigmoid_multilabel(pkg, dev):
    """Activations(sigmoid=True) + AsDiscrete(threshold_values=True) on a 4-in / 3-out model (the multi-label script)"""
    hip = _hip_model(pkg, dev, dict(C1, in_channels=4, out_channels=3))
    hip.precision = "fp32"
    inferer = pkg.SlidingWindowInferer(ROI, 4, overlap=0.25)
    x = _volume((48, 40, 56), 1, channels=4, seed=61).to(dev)
    v = inferer(x, hip)
    got = inferer(x, hip, post="sigmoid")
    want = (torch.sigmoid(v) >= 0.5).float()
    clear = v.abs() > 1e-6
    excluded = 1.0 - clear.float().mean().item()
    print(f"post='sigmoid': {excluded:.3e} of the voxels have |logit| <= 1e-6 and are excluded")
    assert excluded < 1e-4
    assert got.shape == v.shape and torch.equal(got[clear], want[clear])
    assert 0.01 < got.mean().item() < 0.99


# ---------------------------------------------------------------------------------------------- 5. weight freshness
def test_captured_inferer_follows_every_weight_update(pkg, dev):
    torch.manual_seed(11)
    model = pkg.UNETRLogits(**C1).to(dev)
    model.precision = "bf16"
    flat = model.use_flat_buffers()
    x = _volume((32, 48, 80), 1, seed=70).to(dev)           # 6 windows: one full row and a tail of 2 -> two graphs
    inferer = pkg.SlidingWindowInferer(ROI, 4, overlap=0.25, mode="gaussian")

    def check(tag, net=model, inf=inferer):
        got = inf(x, net)                                   # the captured route first: nothing eager has refreshed anything for it
        want = pkg.sliding_window_inference(x, ROI, 4, net, mode="gaussian")
        assert torch.equal(got, want), tag
        return got

    before = check("initial")
    assert inferer.stats["captures"] == 2
    # (a) three captured training steps with this package's AdamW: the copies are optimizer-maintained
    opt = pkg.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-5, flat=flat)
    crit = pkg.DiceCELoss(to_onehot_y=True, softmax=True)
    g = torch.Generator().manual_seed(3)
    xb = torch.randn(2, 1, 32, 32, 32, generator=g).to(dev)
    yb = torch.randint(0, 2, (2, 1, 32, 32, 32), generator=g).float().to(dev)
    step = pkg.TrainStep(model, crit, opt, xb, yb)
    for _ in range(3):
        step.run()
    after = check("TrainStep + AdamW")
    assert relerr(after, before) > 1e-3, "the weights did not move: the check above proves nothing"
    captures = inferer.stats["captures"]
    # (b) load_state_dict of perturbed weights
    g = torch.Generator().manual_seed(4)
    sd = {k: v.detach().cpu() * (1.0 + 0.05 * torch.randn(v.shape, generator=g)) for k, v in model.state_dict().items()}
    model.load_state_dict(sd, strict=True)
    loaded = check("load_state_dict")
    assert relerr(loaded, after) > 1e-3
    # (d) a raw .data write followed by invalidate_weight_shadows()
    with torch.no_grad():
        model.vit.blocks[0].mlp.linear1.weight.data.mul_(1.5)
        model.decoder2.conv_block.conv1.conv.weight.data.mul_(-0.5)
    pkg.invalidate_weight_shadows()
    raw = check(".data write + invalidate_weight_shadows")
    assert relerr(raw, loaded) > 1e-3
    step.run()                                               # and training goes on next to it
    check("TrainStep after the raw write")
    assert inferer.stats["captures"] == captures, "no buffer moved: nothing had to be captured again"
    pkg.functional.clear_grad_sinks()
    # (c) a torch optimizer on a non-flat model
    torch.manual_seed(12)
    plain = pkg.UNETRLogits(**C1).to(dev)
    plain.precision = "bf16"
    inf2 = pkg.SlidingWindowInferer(ROI, 4, overlap=0.25, mode="gaussian")
    first = check("non-flat initial", plain, inf2)
    topt = torch.optim.AdamW(plain.parameters(), lr=1e-3)
    crit(plain(xb), yb).backward()
    topt.step()
    topt.zero_grad(set_to_none=True)
    second = check("torch.optim.AdamW", plain, inf2)
    assert relerr(second, first) > 1e-3


# ---------------------------------------------------------------------------------------------- 6. other callables, tails
@pytest.mark.parametrize("size,batch,overlap,n", [c for c in CASES if c[0] in ((32, 48, 80), (32, 32, 56)) or c[3] == 3] + [CASES[0]])
def test_plain_callable_runs_the_batched_kernels_eagerly(pkg, dev, size, batch, overlap, n):
    hip = _hip_model(pkg, dev, C1)
    hip.precision = "fp32"
    predictor = lambda w: hip(w)                            # returns the (enc4, logits) tuple: the last element is taken
    x = _volume(size, batch, seed=80).to(dev)
    for mode in ("constant", "gaussian"):
        inferer = pkg.SlidingWindowInferer(ROI, n, overlap=overlap, mode=mode)
        got = inferer(x, predictor)
        assert torch.equal(got, pkg.sliding_window_inference(x, ROI, n, predictor, overlap=overlap, mode=mode))
        assert inferer.stats["captures"] == 0 and inferer.stats["replays"] == 0 and inferer.stats["eager_rows"] > 0


def test_non_constant_padding_mode(pkg, dev):
    hip = _hip_model(pkg, dev, C1)
    hip.precision = "fp32"
    x = _volume((24, 40, 28), 1, seed=81).to(dev)
    inferer = pkg.SlidingWindowInferer(ROI, 4, padding_mode="replicate")
    want = pkg.sliding_window_inference(F.pad(x, (2, 2, 0, 0, 4, 4), mode="replicate"), ROI, 4, hip)[:, :, 4:28, :, 2:30]
    assert torch.equal(inferer(x, hip), want)
    inferer = pkg.SlidingWindowInferer(ROI, 4, cval=2.5)
    assert torch.equal(inferer(x, hip), pkg.sliding_window_inference(x, ROI, 4, hip, cval=2.5))
