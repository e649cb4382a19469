"""Mirror test-time augmentation and model ensembling in SlidingWindowInferer on the GPU: the flip in the gather and in the
accumulate through the C ABI (bit for bit against torch.flip around the unflipped yardsticks), the activation inside the accumulate
against float64, the whole call against the float64 reference of tests/tta_ref.py with a derived bound, identity with the inferer
without the new arguments, captured == eager with a real model and an ensemble, the post forms, and the kernels inside red zones."""
import pytest
import torch
import torch.nn.functional as F

from guard import Guard, poison_workspace
from test_inference_gpu import _descriptor, _hip_model, _table, _volume
from test_model_gpu import C1
from tta_ref import activate, flip, ref_tta_sliding_window

pytestmark = pytest.mark.gpu

MASKS = list(range(8))
U = 2.0 ** -24


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------- 1. gather through the C ABI
GATHER = [
    ((20, 22, 26), (8, 12, 16), [(0, 0, 0), (12, 10, 10), (3, 1, 5)]),      # aligned quads, non-cubic; x corners 10 and 5 are no multiple of 4
    ((9, 7, 13), (5, 6, 7), [(0, 0, 0), (4, 1, 6), (2, 0, 3)]),             # scalar path
    ((6, 20, 10), (8, 12, 16), [(0, 0, 0), (0, 8, 0), (0, 3, 0)]),          # overhang on z and x: constant padding inside the gather
]


@pytest.mark.parametrize("in_size,roi,corners", GATHER)
def test_gather_batch_mirrors_the_window(pkg, dev, in_size, roi, corners):
    B, Cin, cval = 2, 2, -1.5
    x = _volume(in_size, B, channels=Cin, seed=150).to(dev)
    pads = [max(r - s, 0) for r, s in zip(roi, in_size)]
    lo = [p // 2 for p in pads]
    padded = F.pad(x, (lo[2], pads[2] - lo[2], lo[1], pads[1] - lo[1], lo[0], pads[0] - lo[0]), value=cval)
    D, H, W = padded.shape[2:]
    n = 4
    slots = [(k % B,) + c for k, c in enumerate(corners)]
    table = _table(pkg, dev, [slots] * len(MASKS))
    table[:, 1] = torch.tensor(MASKS, dtype=torch.int32, device=dev)          # one mask per table row
    desc = _descriptor(pkg, dev, in_=x.data_ptr(), table=table.data_ptr(), B=B, Cin=Cin, C=1, Di=in_size[0], Hi=in_size[1],
                       Wi=in_size[2], D=D, H=H, W=W, pz=lo[0], py=lo[1], px=lo[2], cval=cval, rows=len(MASKS), cursor=-1)
    for mask in MASKS:
        dst = torch.full((n, Cin, *roi), 7.0, device=dev)
        pkg._capi.call("unetr_sw_advance", desc.data_ptr(), _stream())
        pkg._capi.call("unetr_sw_gather_batch", desc.data_ptr(), dst.data_ptr(), n, Cin, *roi, _stream())
        torch.cuda.synchronize()
        for j, (b, z, y, xx) in enumerate(slots):
            win = padded[b:b + 1, :, z:z + roi[0], y:y + roi[1], xx:xx + roi[2]]
            assert torch.equal(dst[j:j + 1], flip(win, mask)), (mask, j)
        assert bool((dst[len(slots):] == cval).all()), mask            # inactive slots
    # the cursor is past the table now: nothing is touched; rewound, row 0 (mask 0) comes again
    dst = torch.full((n, Cin, *roi), 7.0, device=dev)
    pkg._capi.call("unetr_sw_advance", desc.data_ptr(), _stream())
    pkg._capi.call("unetr_sw_gather_batch", desc.data_ptr(), dst.data_ptr(), n, Cin, *roi, _stream())
    assert bool((dst == 7.0).all())
    pkg._capi.call("unetr_sw_rewind", desc.data_ptr(), _stream())
    pkg._capi.call("unetr_sw_advance", desc.data_ptr(), _stream())
    pkg._capi.call("unetr_sw_gather_batch", desc.data_ptr(), dst.data_ptr(), n, Cin, *roi, _stream())
    b, z, y, xx = slots[1]
    assert torch.equal(dst[1], padded[b, :, z:z + roi[0], y:y + roi[1], xx:xx + roi[2]])


# ---------------------------------------------------------------------------------------------- 2. accumulate through the C ABI
# (volume, roi, rows of): 32 windows in rows of 3, tail of 2, x corners 0 and 6 | 16 windows, tail of 1, scalar | 8 windows, tail of 2
ACCUMULATE = [((20, 16, 22), (8, 12, 16), 3), ((7, 7, 10), (5, 6, 7), 3), ((8, 26, 16), (8, 12, 16), 3)]


@pytest.mark.parametrize("with_imp", [True, False])
@pytest.mark.parametrize("size,roi,n", ACCUMULATE)
def test_accumulate_batch_unflips_the_prediction(pkg, dev, size, roi, n, with_imp):
    B, C = 2, 3
    D, H, W = size
    g = torch.Generator().manual_seed(177)
    imp = (torch.rand(*roi, generator=g) + 0.05).to(dev) if with_imp else None          # random, not symmetric
    table_cpu, counts = pkg.inference.plan_window_table(B, size, roi, 0.5, n, flips=MASKS)
    assert counts[-1] < n and len(counts) % len(MASKS) == 0
    table = table_cpu.to(dev)
    out_a = torch.zeros(B, C, D, H, W, device=dev)
    cnt_a = torch.zeros(B, D, H, W, device=dev)
    out_b, cnt_b = torch.zeros_like(out_a), torch.zeros_like(cnt_a)
    desc = _descriptor(pkg, dev, out=out_a.data_ptr(), count=cnt_a.data_ptr(), table=table.data_ptr(), B=B, Cin=1, C=C,
                       Di=D, Hi=H, Wi=W, D=D, H=H, W=W, rows=len(counts), cursor=-1)
    s = _stream()
    ip = imp.data_ptr() if imp is not None else None
    keep = []
    for r, m in enumerate(counts):
        seg = torch.randn(n, C, *roi, generator=g).to(dev)
        mask = int(table_cpu[r, 1])
        assert mask == MASKS[r % len(MASKS)]
        pkg._capi.call("unetr_sw_advance", desc.data_ptr(), s)
        pkg._capi.call("unetr_sw_accumulate_batch", desc.data_ptr(), seg.data_ptr(), ip, n, C, *roi, s)
        back = flip(seg, mask).contiguous()
        keep.append((seg, back))
        for j in range(m):
            b, z, y, x = table_cpu[r, 4 + 4 * j:8 + 4 * j].tolist()
            pkg._capi.call("unetr_sw_accumulate", back[j].data_ptr(), ip, out_b[b].data_ptr(), cnt_b[b].data_ptr(), C, *roi, D, H, W,
                           z, y, x, s)
    torch.cuda.synchronize()
    assert torch.equal(cnt_a, cnt_b) and torch.equal(out_a, out_b)
    assert float(cnt_a.min()) > 0


# ---------------------------------------------------------------------------------------------- 3. activation in the accumulate
def _activation_errors(pkg, dev, C, roi, act, mask):
    """One row of three overlapping windows: max |sums - float64 sums| of (the kernel's activation, torch's fp32 activation followed
    by unetr_sw_accumulate)."""
    size = tuple(r + r // 2 for r in roi)
    D, H, W = size
    corners = [(0, 0, 0), (roi[0] // 2, roi[1] // 2, roi[2] // 2), (0, roi[1] // 2, 3)]
    g = torch.Generator().manual_seed(300 + C)
    imp = torch.rand(*roi, generator=g) + 0.05
    seg = torch.randn(4, C, *roi, generator=g) * 4
    table = _table(pkg, dev, [[(0,) + c for c in corners]])
    table[0, 1] = mask
    out_a = torch.zeros(1, C, D, H, W, device=dev)
    cnt_a = torch.zeros(1, D, H, W, device=dev)
    out_b, cnt_b = torch.zeros_like(out_a), torch.zeros_like(cnt_a)
    desc = _descriptor(pkg, dev, out=out_a.data_ptr(), count=cnt_a.data_ptr(), table=table.data_ptr(), B=1, Cin=1, C=C, Di=D, Hi=H,
                       Wi=W, D=D, H=H, W=W, rows=1, cursor=-1, activation={"softmax": 1, "sigmoid": 2}[act])
    seg_d, imp_d = seg.to(dev), imp.to(dev)
    s = _stream()
    pkg._capi.call("unetr_sw_advance", desc.data_ptr(), s)
    pkg._capi.call("unetr_sw_accumulate_batch", desc.data_ptr(), seg_d.data_ptr(), imp_d.data_ptr(), 4, C, *roi, s)
    back = flip(activate(seg_d, act), mask).contiguous()                 # torch's own fp32 softmax / sigmoid on the same device
    ref = torch.zeros(C, D, H, W, dtype=torch.float64)
    back64 = flip(activate(seg.double(), act), mask)
    for j, (z, y, x) in enumerate(corners):
        pkg._capi.call("unetr_sw_accumulate", back[j].data_ptr(), imp_d.data_ptr(), out_b[0].data_ptr(), cnt_b[0].data_ptr(), C, *roi,
                       D, H, W, z, y, x, s)
        ref[:, z:z + roi[0], y:y + roi[1], x:x + roi[2]] += imp.double() * back64[j]
    torch.cuda.synchronize()
    assert torch.equal(cnt_a, cnt_b)
    return (out_a[0].cpu().double() - ref).abs().max().item(), (out_b[0].cpu().double() - ref).abs().max().item()


@pytest.mark.parametrize("mask", [0, 7])
@pytest.mark.parametrize("act", ["softmax", "sigmoid"])
@pytest.mark.parametrize("roi", [(8, 12, 16), (5, 6, 7)])
@pytest.mark.parametrize("C", [2, 16])
def test_activation_inside_the_accumulate(pkg, dev, C, roi, act, mask):
    """Allowed error: 4 x the error torch's own fp32 softmax / sigmoid followed by unetr_sw_accumulate shows against the same
    float64 sums (the factor allows for expf and the divide each differing from torch's by a few ulp, and for the fma roundings of
    the blend).  Measured on an MI355X (profiles/tta_inferer.txt lists all 16 cases), max |sums - float64 sums| of the kernel and
    of the yardstick: softmax 1.238e-07 .. 3.052e-07, sigmoid 1.268e-07 .. 2.354e-07, and in every case the two agree to the printed
    digits (e.g. softmax C=16 (8, 12, 16) mask 0: 3.052e-07 and 3.052e-07; sigmoid C=2 (5, 6, 7) mask 7: 1.268e-07 and 1.268e-07) --
    the largest error is the rounding of the blend's sums, which both routes perform with the same fp32 operations."""
    e_new, e_torch = _activation_errors(pkg, dev, C, roi, act, mask)
    print(f"activation {act} C={C} roi={roi} mask={mask}: kernel {e_new:.3e}, torch fp32 + unetr_sw_accumulate {e_torch:.3e}")
    assert e_torch > 0 and e_new <= 4 * e_torch


# ---------------------------------------------------------------------------------------------- 4. end to end, plain callables
ROI16 = (16, 16, 16)


def _ramp_predictor(seed):
    """channel c = x * R_c + S_c with fixed integer ramps over the position in the FORWARDED window: exact in fp32 for integer x,
    the same on the GPU and in float64, and not flip-equivariant"""
    z, y, x = torch.meshgrid(torch.arange(16), torch.arange(16), torch.arange(16), indexing="ij")
    R = torch.stack([(z + 2 * y + 3 * x + c * seed) % 5 - 2 for c in range(3)]).float()
    S = torch.stack([(3 * z + 5 * y + (c + 2) * x + seed) % 7 - 3 for c in range(3)]).float()
    cache = {}

    def predict(w):
        key = (w.device, w.dtype)
        if key not in cache:
            cache[key] = (R.to(w), S.to(w))
        r, s = cache[key]
        return w[:, :1] * r + s
    return predict


def _coverage(pkg, B, size, roi, overlap, n):
    """largest number of windows that cover one voxel, from the planned table"""
    table, counts = pkg.inference.plan_window_table(B, size, roi, overlap, n)
    cov = torch.zeros(B, *size, dtype=torch.int32)
    for r, m in enumerate(counts):
        for j in range(m):
            b, z, y, x = table[r, 4 + 4 * j:8 + 4 * j].tolist()
            cov[b, z:z + roi[0], y:y + roi[1], x:x + roi[2]] += 1
    return int(cov.max())


def _exact_case(pkg, dev, size, overlap, mode, flips, models, use_graph=True):
    B, n = 2, 3
    g = torch.Generator().manual_seed(400)
    x = torch.randint(-8, 9, (B, 1, *size), generator=g).float()
    nets = [_ramp_predictor(1), _ramp_predictor(4)][:models]
    masks = pkg.inference.flip_masks(flips)
    imp = pkg.inference.importance_map(ROI16, mode)                     # the fp32 weights the GPU blends with, taken as given
    ref = ref_tta_sliding_window(x, ROI16, n, nets, masks, overlap=overlap, importance=imp)
    inferer = pkg.SlidingWindowInferer(ROI16, n, overlap=overlap, mode=mode, tta_flips=flips, use_graph=use_graph)
    got = inferer(x.to(dev), nets if models > 1 else nets[0])
    padded = [max(s, r) for s, r in zip(size, ROI16)]
    terms = _coverage(pkg, B, padded, ROI16, overlap, n) * len(masks) * models
    seg_max = 8 * 2 + 3
    err = (got.cpu().double() - ref).abs().max().item()
    bound = (2 * terms + 2) * U * seg_max
    print(f"{size} overlap={overlap} {mode} flips={flips} models={models}: n={terms}, max err {err:.3e}, bound {bound:.3e}")
    assert got.shape == ref.shape == (B, 3, *size)
    assert err <= bound
    rows = len(pkg.inference.plan_window_table(B, padded, ROI16, overlap, n)[1])
    assert inferer.stats == dict(captures=0, recaptures=0, replays=0, eager_rows=rows * len(masks) * models)
    return got


@pytest.mark.parametrize("models", [1, 2])
@pytest.mark.parametrize("flips", ["all", [(0,), (1, 2)]])
@pytest.mark.parametrize("mode", ["constant", "gaussian"])
@pytest.mark.parametrize("overlap", [0.25, 0.5])
def test_end_to_end_against_float64(pkg, dev, overlap, mode, flips, models):
    """|got - ref| <= (2n + 2) * 2^-24 * max|seg|, n = the largest number of (model, window, flip) terms covering a voxel: the
    window predictions are exact, the sum of n fma roundings in the numerator and n roundings in the denominator each move the
    quotient by at most n * 2^-24 * max|seg| to first order, the divide by one more; one is left for the second-order terms."""
    _exact_case(pkg, dev, (20, 24, 36), overlap, mode, flips, models)


def test_end_to_end_volume_smaller_than_the_window(pkg, dev):
    got = _exact_case(pkg, dev, (12, 24, 36), 0.25, "gaussian", "all", 2)
    assert got.shape == (2, 3, 12, 24, 36)


def test_flips_are_not_a_no_op(pkg, dev):
    """the ramp predictors are not flip-equivariant: the augmented result differs from the plain one by far more than the bound"""
    x = torch.randint(-8, 9, (1, 1, 20, 24, 36), generator=torch.Generator().manual_seed(401)).float().to(dev)
    net = _ramp_predictor(1)
    plain = pkg.SlidingWindowInferer(ROI16, 3, overlap=0.5)(x, net)
    for flips in ([(0,)], [(1,)], [(2,)]):
        assert (pkg.SlidingWindowInferer(ROI16, 3, overlap=0.5, tta_flips=flips)(x, net) - plain).abs().max().item() > 1.0


@pytest.mark.parametrize("act", ["softmax", "sigmoid"])
def test_end_to_end_with_activation(pkg, dev, act):
    """non-exact predictors; yardstick of test_activation_inside_the_accumulate: 4 x the error of the same inferer without
    ``activation`` whose predictors apply torch's fp32 softmax / sigmoid themselves"""
    B, n, size = 2, 3, (20, 24, 36)
    x = _volume(size, B, seed=402)
    nets = [lambda w: torch.cat([w * 1.3, torch.sin(w * 2) * 3, -w * 0.7 + 0.2], 1), lambda w: torch.cat([w * w - 1, w * 0.5, torch.cos(w)], 1)]
    imp = pkg.inference.importance_map(ROI16, "gaussian")
    ref = ref_tta_sliding_window(x, ROI16, n, nets, MASKS, activation=act, overlap=0.5, importance=imp)
    new = pkg.SlidingWindowInferer(ROI16, n, overlap=0.5, mode="gaussian", tta_flips="all", activation=act)
    old = pkg.SlidingWindowInferer(ROI16, n, overlap=0.5, mode="gaussian", tta_flips="all")
    got_new = new(x.to(dev), nets)
    got_old = old(x.to(dev), [lambda w, f=f: activate(f(w), act) for f in nets])
    e_new, e_old = (got_new.cpu().double() - ref).abs().max().item(), (got_old.cpu().double() - ref).abs().max().item()
    print(f"end to end, activation {act}: in the kernel {e_new:.3e}, torch in the predictor {e_old:.3e}")
    assert e_old > 0 and e_new <= 4 * e_old
    if act == "softmax":
        assert (got_new.sum(1) - 1).abs().max().item() < 1e-5
        with pytest.raises(NotImplementedError):
            new(x.to(dev), lambda w: w.expand(-1, 17, -1, -1, -1))


# ---------------------------------------------------------------------------------------------- 5. identity
ROI = (32, 32, 32)


@pytest.mark.parametrize("use_graph", [True, False])
def test_single_empty_flip_is_the_plain_inferer(pkg, dev, use_graph):
    hip = _hip_model(pkg, dev, C1)
    hip.precision = "fp32"
    x = _volume((40, 48, 56), 1, seed=500).to(dev)
    tta = pkg.SlidingWindowInferer(ROI, 4, mode="gaussian", use_graph=use_graph, tta_flips=[()], activation=None)
    plain = pkg.SlidingWindowInferer(ROI, 4, mode="gaussian", use_graph=use_graph)
    got = tta(x, hip)
    assert torch.equal(got, plain(x, hip))
    assert torch.equal(got, pkg.sliding_window_inference(x, ROI, 4, hip, mode="gaussian"))
    assert tta.stats == plain.stats


# ---------------------------------------------------------------------------------------------- 6. captured == eager, real model
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_captured_equals_eager_under_all_flips(pkg, dev, precision):
    hip = _hip_model(pkg, dev, C1)
    hip.precision = precision
    kw = dict(overlap=0.25, mode="gaussian", tta_flips="all")
    graph = pkg.SlidingWindowInferer(ROI, 3, use_graph=True, **kw)
    eager = pkg.SlidingWindowInferer(ROI, 3, use_graph=False, **kw)
    sizes, rows = set(), 0
    for k, size in enumerate([(48, 48, 48), (24, 24, 24)]):
        x = _volume(size, 1, seed=600 + k).to(dev)
        got = graph(x, hip)
        assert torch.equal(got, eager(x, hip)), size
        assert torch.equal(got, eager(x, lambda w: hip(w))), size
        assert torch.equal(graph(x, hip), got), "a second call returns other bits"
        counts = pkg.inference.plan_window_table(1, [max(v, 32) for v in size], ROI, 0.25, 3)[1]
        sizes.update(counts)
        rows += len(counts)
        assert graph.stats["captures"] == len(sizes)                      # one graph per row size, whatever the number of flips
    assert sizes == {3, 2, 1}
    assert graph.stats == dict(captures=3, recaptures=0, replays=2 * rows * 8, eager_rows=0)
    assert eager.stats == dict(captures=0, recaptures=0, replays=0, eager_rows=2 * rows * 8)


def test_captured_ensemble_of_two_models(pkg, dev):
    a, b = _hip_model(pkg, dev, C1, seed=3), _hip_model(pkg, dev, C1, seed=8)
    a.precision = b.precision = "bf16"
    kw = dict(overlap=0.25, mode="gaussian", tta_flips="all")
    graph = pkg.SlidingWindowInferer(ROI, 3, use_graph=True, **kw)
    eager = pkg.SlidingWindowInferer(ROI, 3, use_graph=False, **kw)
    x = _volume((48, 48, 48), 1, seed=610).to(dev)
    got = graph(x, [a, b])
    assert torch.equal(got, eager(x, (a, b)))
    assert torch.equal(got, eager(x, [lambda w: a(w), lambda w: b(w)]))
    assert torch.equal(graph(x, [a, b]), got), "a second call returns other bits"
    assert graph.stats == dict(captures=2 * 2, recaptures=0, replays=2 * 2 * 3 * 8, eager_rows=0)       # row sizes {3, 2}, 3 rows
    single = graph(x, a)
    assert (got - single).abs().max().item() > 1e-3, "the second model did not contribute"
    with pytest.raises(ValueError):
        graph(x, [a, _hip_model(pkg, dev, dict(C1, out_channels=3))])


# ---------------------------------------------------------------------------------------------- 7. post forms
def _tie_predictor(w):
    return torch.cat([w * 0.5, w, w, -w], 1)              # channels 1 and 2 identical; all equal where the input is 0


@pytest.mark.parametrize("act", [None, "sigmoid"])
def test_post_sigmoid_thresholds_the_average(pkg, dev, act):
    x = torch.randint(-3, 4, (1, 1, 20, 24, 36), generator=torch.Generator().manual_seed(700)).float().to(dev)
    inferer = pkg.SlidingWindowInferer(ROI16, 3, overlap=0.5, mode="gaussian", tta_flips="all", activation=act)
    nets = [_tie_predictor, lambda w: _tie_predictor(w) * 0.25]
    v = inferer(x, nets)
    got = inferer(x, nets, post="sigmoid")
    thr = 0.5 if act == "sigmoid" else 0.0
    assert got.shape == v.shape and torch.equal(got, (v >= thr).float())
    assert int((v == thr).sum()) > 1000 and 0.05 < got.mean().item() < 0.95          # exact hits of the threshold are in the data


@pytest.mark.parametrize("act", [None, "softmax"])
def test_post_argmax_and_onehot_of_the_average(pkg, dev, act):
    x = torch.randint(-3, 4, (1, 1, 20, 24, 36), generator=torch.Generator().manual_seed(701)).float().to(dev)
    inferer = pkg.SlidingWindowInferer(ROI16, 3, overlap=0.5, mode="gaussian", tta_flips="all", activation=act)
    v = inferer(x, _tie_predictor)
    assert torch.equal(v[:, 1], v[:, 2])
    am = v.argmax(dim=1)
    assert set(am.unique().tolist()) == {0, 1, 3}                            # first maximum on ties: never channel 2
    assert torch.equal(inferer(x, _tie_predictor, post="argmax"), am.unsqueeze(1).float())
    assert torch.equal(inferer(x, _tie_predictor, post="onehot"), F.one_hot(am, 4).movedim(-1, 1).float())


def test_post_sigmoid_after_softmax_raises(pkg, dev):
    x = torch.zeros(1, 1, 20, 24, 36, device=dev)
    with pytest.raises(ValueError):
        pkg.SlidingWindowInferer(ROI16, 3, activation="softmax")(x, _tie_predictor, post="sigmoid")


# ---------------------------------------------------------------------------------------------- 8. red zones
@pytest.mark.parametrize("in_size,roi,corners", GATHER)
def test_guarded_gather(pkg, dev, in_size, roi, corners):
    poison_workspace(pkg.functional, dev)
    with Guard(dev) as gd:
        test_gather_batch_mirrors_the_window(pkg, dev, in_size, roi, corners)
    assert gd.check() > 0


@pytest.mark.parametrize("with_imp", [True, False])
@pytest.mark.parametrize("size,roi,n", ACCUMULATE)
def test_guarded_accumulate(pkg, dev, size, roi, n, with_imp):
    poison_workspace(pkg.functional, dev)
    with Guard(dev) as gd:
        test_accumulate_batch_unflips_the_prediction(pkg, dev, size, roi, n, with_imp)
    assert gd.check() > 0
