"""The segmentation loss family (csrc/seg_loss.hip behind SegLoss and its presets) against the float64 reference of
tests/segloss_ref.py: the three terms and the logits gradient, under an upstream gradient that is not 1.

Shapes (B, C, S), V = S^3, the smallest at which each path can go wrong (forward chunk = 4096 voxels, 16-byte loads when V % 4 == 0;
backward block = 256 voxels, one per thread):
  (1, 2, 17)   V = 4913: odd V, so the forward's scalar loop; two forward chunks, the second partial; a partial last backward block
  (2, 4, 16)   V = 4096: exactly one full chunk, 16-byte path
  (2, 3, 24)   V = 13824: several chunks, the last one partial, 16-byte path
  (1, 14, 12)  the 14 classes of BTCV
  (1, 1, 17)   one channel: multilabel mode only
  (1, 16, 8)   the channel cap

Bounds: those of test_ops_gpu.py::test_dicece for this kernel family -- relerr < 1e-5 on each term, < 1e-4 on the gradient
(util.relerr: max |a-b| / max |b|).  One term is legitimately zero and is compared by absolute error < 1e-6 instead: the cross
entropy of a ONE-channel input (case "ml-1ch-dice-ce"), where softmax is 1 and -log 1 = 0 in the reference and in the kernel."""
import pytest
import torch

from guard import Guard, poison_workspace
from segloss_ref import segloss_ref
from util import relerr

pytestmark = pytest.mark.gpu

ONEHOT = dict(to_onehot_y=True, softmax=True)
MULTI = dict(to_onehot_y=False, sigmoid=True)
A, B4, C3, D14, E1, F16 = (1, 2, 17), (2, 4, 16), (2, 3, 24), (1, 14, 12), (1, 1, 17), (1, 16, 8)
W4, W3 = [0.2, 1.0, 3.0, 0.5], [0.5, 2.0, 1.25]
W14 = [0.1 + 0.15 * i for i in range(14)]


def case(id, shape, mode, label=None, zero_voxel_term=False, **kw):
    return pytest.param(shape, mode, label, zero_voxel_term, kw, id=id)


CASES = [
    # every region kind, without and with a voxel term
    case("oh-dice", A, "oh", voxel="none"),
    case("oh-dice-ce", A, "oh"),
    case("ml-jaccard", B4, "ml", region="jaccard", voxel="none"),
    case("oh-jaccard-focal", C3, "oh", region="jaccard", voxel="focal"),
    case("oh-tversky", B4, "oh", region="tversky", voxel="none", alpha=0.3, beta=0.7),
    case("ml-tversky-ce", C3, "ml", region="tversky", alpha=0.7, beta=0.3),
    case("oh-gdl-square", C3, "oh", region="generalized_dice", voxel="none"),
    case("ml-gdl-simple-focal", B4, "ml", region="generalized_dice", voxel="focal", w_type="simple"),
    case("oh-gdl-uniform-ce-btcv", D14, "oh", region="generalized_dice", w_type="uniform"),
    case("ml-gdl-square-btcv", D14, "ml", region="generalized_dice", voxel="none"),
    case("oh-ce", A, "oh", region="none"),
    case("ml-ce", B4, "ml", region="none"),
    # include_background=False, squared_pred, batch, lambdas: each in each mode
    case("oh-nobg-dice-ce", C3, "oh", include_background=False),
    case("ml-nobg-dice-focal", B4, "ml", include_background=False, voxel="focal"),
    case("oh-nobg-gdl", B4, "oh", include_background=False, region="generalized_dice", voxel="none"),
    case("oh-squared-dice", B4, "oh", squared_pred=True, voxel="none"),
    case("ml-squared-jaccard-ce", C3, "ml", squared_pred=True, region="jaccard"),
    case("oh-squared-jaccard", A, "oh", squared_pred=True, region="jaccard", voxel="none"),
    case("ml-squared-dice", A, "ml", squared_pred=True, voxel="none"),
    case("oh-batch-dice-ce", C3, "oh", batch=True),
    case("ml-batch-tversky", B4, "ml", batch=True, region="tversky", voxel="none", alpha=0.4, beta=0.6),
    case("oh-batch-gdl", B4, "oh", batch=True, region="generalized_dice", voxel="none"),
    case("ml-batch-jaccard-focal", C3, "ml", batch=True, region="jaccard", voxel="focal"),
    case("oh-lambdas", A, "oh", lambda_region=0.3, lambda_voxel=1.7),
    case("ml-lambdas", B4, "ml", voxel="focal", lambda_region=2.0, lambda_voxel=0.25),
    # weighted cross entropy
    case("oh-weighted-ce", B4, "oh", class_weight=W4),
    case("oh-weighted-ce-btcv", D14, "oh", class_weight=W14, include_background=False),
    # focal: gamma 0 and 2, without and with weights
    case("oh-focal-g0", B4, "oh", region="none", voxel="focal", gamma=0.0),
    case("ml-focal-g0-weights", C3, "ml", region="none", voxel="focal", gamma=0.0, class_weight=W3),
    case("oh-focal-g2-weights", C3, "oh", region="none", voxel="focal", gamma=2.0, class_weight=W3),
    case("ml-focal-g2", A, "ml", region="none", voxel="focal", gamma=2.0),
    case("oh-focal-g2-nobg-btcv", D14, "oh", region="none", voxel="focal", gamma=2.0, include_background=False, class_weight=W14),
    # ignore_index with about 30 % of the voxels ignored
    case("oh-ignore-weighted-dice-ce", C3, "oh", label="ignore", class_weight=W3, ignore_index=255),
    case("oh-ignore-dice-focal-scalar", A, "oh", label="ignore", voxel="focal", ignore_index=255),
    case("oh-ignore-gdl-ce", B4, "oh", label="ignore", region="generalized_dice", ignore_index=255),
    case("oh-ignore-negative-index-batch", C3, "oh", label="ignore", batch=True, region="tversky", ignore_index=-1),
    # a volume that lacks one class entirely; a batch item that is one class
    case("oh-absent-class-dice-ce", C3, "oh", label="absent"),
    case("oh-absent-class-gdl", C3, "oh", label="absent", region="generalized_dice", voxel="none"),
    case("oh-single-class-item-dice-ce", B4, "oh", label="single"),
    case("oh-single-class-item-gdl-focal", B4, "oh", label="single", region="generalized_dice", voxel="focal", w_type="simple"),
    case("ml-empty-item-gdl", B4, "ml", label="empty", region="generalized_dice", voxel="none"),
    # one channel (multilabel only) and the channel cap
    case("ml-1ch-dice-ce", E1, "ml", zero_voxel_term=True),
    case("ml-1ch-dice-focal", E1, "ml", voxel="focal"),
    case("oh-16ch-dice-ce", F16, "oh"),
    case("ml-16ch-jaccard-focal", F16, "ml", region="jaccard", voxel="focal"),
    case("ml-btcv-dice-ce", D14, "ml"),
]

_INPUTS = {}


def inputs(shape, mode, label):
    """seeded logits and target of a case (CPU, shared between the cases that use them, never modified)"""
    key = (shape, mode, label)
    if key not in _INPUTS:
        B, C, S = shape
        gen = torch.Generator().manual_seed(1000 * C + S)
        logits = torch.randn(B, C, S, S, S, generator=gen) * 2
        if mode == "ml":
            t = (torch.rand(B, C, S, S, S, generator=gen) < 0.35).float()      # channels overlap, many voxels are all-zero
            if label == "empty":
                t[0] = 0
        else:
            t = torch.randint(0, C, (B, 1, S, S, S), generator=gen).float()
            if label == "ignore":
                t[torch.rand(t.shape, generator=gen) < 0.3] = 255.0
            elif label == "absent":
                t[t == 1] = 2.0
            elif label == "single":
                t[0] = 2.0
        _INPUTS[key] = (logits, t)
    return _INPUTS[key]


def reference(logits, target, kw):
    z = logits.clone().requires_grad_(True)
    R, X = segloss_ref(z, target, **kw)
    loss = kw.get("lambda_region", 1.0) * R * (kw.get("region", "dice") != "none") + \
        kw.get("lambda_voxel", 1.0) * X * (kw.get("voxel", "ce") != "none")
    (loss * 0.37).backward()
    return loss.detach(), R.detach(), X.detach(), z.grad


def close(got, want, zero=False):
    if zero:
        assert abs(float(want)) < 1e-12
        return abs(float(got.detach()) - float(want)) < 1e-6
    return relerr(got, want) < 1e-5


def run_case(pkg, dev, shape, mode, label, zero_voxel_term, kw):
    kw = dict(ONEHOT if mode == "oh" else MULTI, **kw)
    logits, target = inputs(shape, mode, label)
    if kw.get("ignore_index") == -1:
        target = torch.where(target == 255.0, torch.full_like(target, -1.0), target)
    loss, R, X, grad = reference(logits, target, kw)
    crit = pkg.SegLoss(**kw)
    ld = logits.to(dev).requires_grad_(True)
    t = crit.terms(ld, target.to(dev))
    print(f"terms {t.tolist()} reference {[float(loss), float(R), float(X)]}")
    assert close(t[0], loss) and close(t[1], R) and close(t[2], X, zero_voxel_term), (t.tolist(), float(loss), float(R), float(X))
    (t[0] * 0.37).backward()
    e = relerr(ld.grad, grad)
    print(f"gradient relerr {e:.3e}")
    assert e < 1e-4
    return crit, ld, t


@pytest.mark.parametrize("shape,mode,label,zero_voxel_term,kw", CASES)
def test_terms_and_gradient(pkg, dev, shape, mode, label, zero_voxel_term, kw):
    crit, ld, t = run_case(pkg, dev, shape, mode, label, zero_voxel_term, kw)
    # .forward is element 0 of .terms, with the same gradient
    _, target = inputs(shape, mode, label)
    if kw.get("ignore_index") == -1:
        target = torch.where(target == 255.0, torch.full_like(target, -1.0), target)
    l2 = ld.detach().clone().requires_grad_(True)
    loss = crit(l2, target.to(dev))
    assert loss.dim() == 0 and torch.equal(loss.detach(), t[0].detach())
    (loss * 0.37).backward()
    assert torch.equal(l2.grad, ld.grad)
    if label == "ignore":                       # an ignored voxel has no gradient at all
        assert not ld.grad.cpu()[(target == float(kw["ignore_index"])).expand_as(ld)].any()


@pytest.mark.parametrize("mode", ["oh", "ml"])
@pytest.mark.parametrize("shape", [A, C3])
def test_inside_guard_with_poisoned_workspace(pkg, dev, mode, shape):
    """Inputs, outputs and the coefficient buffer between NaN red zones, the scratch buffer poisoned: a read past V, a partial row
    that is consumed without having been written, or an output element that is not written, is a NaN in the result; a write past
    a buffer changes a red zone.  (1, 2, 17) runs the forward's scalar loop with a partial second chunk and a partial last backward
    block, (2, 3, 24) the 16-byte path with a partial last chunk."""
    kw = dict(region="jaccard", voxel="focal", include_background=False, class_weight=[0.5, 2.0, 1.25][:shape[1]])
    poison_workspace(pkg.functional, dev)
    with Guard(dev) as gd:
        run_case(pkg, dev, shape, mode, None, False, kw)
        torch.cuda.synchronize()
    assert gd.check() > 0


@pytest.mark.parametrize("mode", ["oh", "ml"])
def test_defaults_agree_with_dicece(pkg, dev, mode):
    kw = ONEHOT if mode == "oh" else MULTI
    logits, target = inputs(C3, mode, None)
    res = []
    for crit in (pkg.DiceCELoss(**kw), pkg.SegLoss(**kw)):
        ld = logits.to(dev).requires_grad_(True)
        t = crit.terms(ld, target.to(dev))
        (t[0] * 0.37).backward()
        res.append((t.detach(), ld.grad))
    for k in range(3):
        assert relerr(res[1][0][k], res[0][0][k]) < 1e-5
    assert relerr(res[1][1], res[0][1]) < 1e-4


@pytest.mark.parametrize("mode", ["oh", "ml"])
def test_unaligned_pointers_take_the_scalar_loop(pkg, dev, mode):
    """V % 4 == 0 but the logits start 4 bytes past a 16-byte boundary: the forward must not issue 16-byte loads; same result as the
    aligned call, to the bounds (the two paths sum in different orders)"""
    kw = dict(ONEHOT if mode == "oh" else MULTI, voxel="focal", class_weight=W4)
    logits, target = inputs(B4, mode, None)
    crit = pkg.SegLoss(**kw)
    res = []
    for shift in (0, 1):
        buf = torch.zeros(logits.numel() + 4, device=dev)
        ld = buf[shift:shift + logits.numel()].view(logits.shape)
        ld.copy_(logits)
        assert ld.is_contiguous() and ld.data_ptr() % 16 == 4 * shift
        ld.requires_grad_(True)
        t = crit.terms(ld, target.to(dev))
        (t[0] * 0.37).backward()
        res.append((t.detach(), ld.grad.clone()))
    for k in range(3):
        assert relerr(res[1][0][k], res[0][0][k]) < 1e-5
    assert relerr(res[1][1], res[0][1]) < 1e-4


def test_reproducible_run_to_run(pkg, dev):
    logits, target = inputs(C3, "oh", None)
    crit = pkg.DiceFocalLoss(**ONEHOT)
    outs = []
    for _ in range(3):
        ld = logits.to(dev).requires_grad_(True)
        t = crit.terms(ld, target.to(dev))
        t[0].backward()
        outs.append((t.detach().clone(), ld.grad.clone()))
    assert all(torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]) for o in outs[1:])


def test_too_many_channels_is_unsupported(pkg, dev):
    logits = torch.zeros(1, 17, 4, 4, 4, device=dev)
    with pytest.raises(RuntimeError, match="unsupported"):
        pkg.SegLoss(**ONEHOT)(logits, torch.zeros(1, 1, 4, 4, 4, device=dev))
    with pytest.raises(RuntimeError, match="unsupported"):
        pkg.DiceFocalLoss(**MULTI)(logits, torch.zeros(1, 17, 4, 4, 4, device=dev))


def test_captured_train_step_with_dice_focal(pkg, dev):
    """TrainStep takes any criterion(logits, y): three captured steps with DiceFocalLoss(include_background=False) on the smallest
    model geometry of test_model_gpu.py (C1, 32^3) give finite losses, the losses of three eager steps from the same state -- bit
    for bit, as test_model_gpu.py::test_staged_backward_equals_single_pass holds its captured and eager forms to each other."""
    from oracle.unetr_oracle import synthetic_volume
    from test_model_gpu import C1
    x, y = synthetic_volume(2, 1, 32, 2, seed=41)
    xd, yd = x.to(dev), y.to(dev)
    res = {}
    for mode in ("graph", "eager"):
        torch.manual_seed(11)
        m = pkg.UNETRLogits(**C1).to(dev)
        m.precision = "bf16"
        flat = m.use_flat_buffers()
        opt = pkg.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-5, flat=flat)
        crit = pkg.DiceFocalLoss(include_background=False, to_onehot_y=True, softmax=True)
        step = pkg.TrainStep(m, crit, opt, xd, yd, use_graph=mode == "graph", warmup=2)
        assert (step.graphs is not None) == (mode == "graph")
        losses = []
        for _ in range(3):
            step.run()
            losses.append(float(step.loss.detach()))
        torch.cuda.synchronize()
        res[mode] = (losses, flat["param"].clone())
        flat["state"].clear()
        del step, opt, m, flat
    print("captured", res["graph"][0], "eager", res["eager"][0])
    assert all(l == l and abs(l) < float("inf") for l in res["graph"][0])
    assert res["graph"][0] == res["eager"][0]
    assert torch.equal(res["graph"][1], res["eager"][1])
