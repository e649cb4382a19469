"""TopKLoss / DiceTopKLoss (csrc/topk_loss.hip on the radix select of csrc/select.hip) against the float64 reference of
tests/topk_ref.py: the loss and the logits gradient, under an upstream gradient of 0.37.

Kernels: the value pass moves 1024 voxels per block, four per thread as 16-byte loads when V % 4 == 0 and the pointers are aligned
(its scalar loop otherwise); the select's histogram passes take 4096 values per workgroup, the sum pass 4096 per block, the backward
256 voxels per block, one per thread.  Shapes (B, C, S), V = S^3, with the input recipe of test_segloss_gpu.py:
  (1, 2, 17)   V = 4913: odd V -> every scalar loop; five value blocks, the last partial; two select workgroups and two sum blocks
  (2, 4, 16)   V = 4096: 16-byte paths, whole blocks everywhere; B*V = 8192 values
  (2, 3, 24)   V = 13824: 16-byte paths, a partial last value block; B*V = 27648 values = seven select workgroups, the last partial
  (1, 14, 12)  the 14 classes of BTCV;   (1, 16, 8)  the channel cap

Bounds: those of test_segloss_gpu.py for this kernel family -- relerr < 1e-5 on the loss, < 1e-4 on the gradient.  A rounding
difference between the kernel's fp32 values and the float64 reference could move one voxel across the threshold and change the
gradient there by about 1/K, so every (input, k) used here keeps the K-th and (K+1)-th largest reference values at least 1e-4
apart, relative (about a thousand fp32 ulps against a few ulps of expf / logf error): `gap_cases()` lists them and
test_topk_cpu.py asserts the precondition over that list without a GPU."""
import pytest
import torch

from guard import Guard, poison_workspace
from test_segloss_gpu import A, B4, C3, D14, F16, MULTI, ONEHOT, W3, W4, inputs
from topk_ref import case_gap, k_count, tie_weights, topk_ref, voxel_values
from util import relerr

pytestmark = pytest.mark.gpu

UP = 0.37
MIN_GAP = 1e-4


def case(id, shape, mode, label, k, **kw):
    return pytest.param(shape, mode, label, k, kw, id=id)


def _table():
    rows = [("a", A, None, None, (10, 12.5)), ("a-ignore", A, "ignore", None, (10, 12.5, 25)), ("b4", B4, None, None, (10, 12.5, 25)),
            ("b4-w", B4, None, W4, (10, 12.5)), ("b4-ignore", B4, "ignore", None, (10, 25)), ("c3", C3, None, None, (12.5, 25)),
            ("c3-w", C3, None, W3, (10,)), ("c3-ignore-w", C3, "ignore", W3, (25,)), ("d14", D14, None, None, (10, 12.5, 25)),
            ("f16", F16, None, None, (10, 12.5, 25))]
    out = []
    for name, shape, label, w, ks in rows:
        for k in ks:
            kw = {}
            if w is not None:
                kw["class_weight"] = w
            if label == "ignore":
                kw["ignore_index"] = 255
            out.append(case(f"oh-{name}-k{k}", shape, "oh", label, float(k), **kw))
    # multilabel form (mask targets, class = first argmax): k picked under the same precondition
    for name, shape, ks in (("a", A, ML_K[A]), ("b4", B4, ML_K[B4]), ("c3", C3, ML_K[C3]), ("d14", D14, ML_K[D14]), ("f16", F16, ML_K[F16])):
        out += [case(f"ml-{name}-k{k}", shape, "ml", None, float(k)) for k in ks]
    return out


ML_K = {A: (12.5, 25), B4: (10, 25), C3: (12.5, 50), D14: (10, 25), F16: (10, 25)}
CASES = _table()
K_ONE = 0.01          # of 4913 voxels: floor(0.49) = 0 -> K = 1


def mode_kw(mode):
    return ONEHOT if mode == "oh" else MULTI


def batch_scope_inputs():
    """(2, 4, 16) with item 0's logits scaled to 5 %: its cross entropies sit near log 4, below the hardest fifth of item 1"""
    logits, target = inputs(B4, "oh", None)
    logits = logits.clone()
    logits[0] *= 0.05
    return logits, target


def tie_inputs():
    """logits drawn from five integer vectors, labels from three classes: at most 15 distinct values, each shared bit for bit (in
    fp32 and in float64) by hundreds of voxels.  V = 17^3, so B*V = 9826 values."""
    gen = torch.Generator().manual_seed(77)
    palette = torch.tensor([[3.0, 0.0, -1.0], [0.0, 2.0, 1.0], [-2.0, 1.0, 4.0], [1.0, 1.0, 1.0], [5.0, -3.0, 0.0]])
    pick = torch.randint(0, 5, (2, 17, 17, 17), generator=gen)
    logits = palette[pick].movedim(-1, 1).contiguous()
    target = torch.randint(0, 3, (2, 1, 17, 17, 17), generator=gen).float()
    return logits, target


def gap_cases():
    """(id, logits, target, k, reference kwargs) of every (input, k) a test below compares with the reference under the bounds --
    the tie case excepted, whose threshold lies inside a group of equal values on purpose"""
    out = []
    for p in CASES:
        shape, mode, label, k, kw = p.values
        logits, target = inputs(shape, mode, label)
        out.append((p.id, logits, target, k, dict(mode_kw(mode), **kw)))
    logits, target = inputs(A, "oh", None)
    out.append(("k-one", logits, target, K_ONE, dict(ONEHOT)))
    logits, target = batch_scope_inputs()
    out.append(("batch-scope", logits, target, 10.0, dict(ONEHOT)))
    return out


def reference(logits, target, k, kw):
    z = logits.clone().requires_grad_(True)
    X = topk_ref(z, target, k=k, **kw)
    (X * UP).backward()
    return X.detach(), z.grad


def run_case(pkg, dev, logits, target, k, kw, ld=None):
    """loss and gradient of TopKLoss(k, **kw) on the device against the reference; returns (criterion, device logits, loss)"""
    assert case_gap(logits, target, k, **kw) >= MIN_GAP
    X, grad = reference(logits, target, k, kw)
    crit = pkg.TopKLoss(k=k, **kw)
    if ld is None:
        ld = logits.to(dev)
    ld.requires_grad_(True)
    loss = crit(ld, target.to(dev))
    assert loss.dim() == 0
    e = relerr(loss, X)
    print(f"loss {float(loss.detach()):.9g} reference {float(X):.9g} relerr {e:.3e}")
    (loss * UP).backward()
    eg = relerr(ld.grad, grad)
    print(f"gradient relerr {eg:.3e}")
    assert e < 1e-5
    assert eg < 1e-4
    return crit, ld, loss


@pytest.mark.parametrize("shape,mode,label,k,kw", CASES)
def test_loss_and_gradient(pkg, dev, shape, mode, label, k, kw):
    logits, target = inputs(shape, mode, label)
    _, ld, _ = run_case(pkg, dev, logits, target, k, dict(mode_kw(mode), **kw))
    g = ld.grad.cpu()
    if label == "ignore":                       # an ignored voxel has no gradient bit set
        assert not g.view(torch.int32)[(target == 255.0).expand_as(g)].any()
    # the gradient is zero outside the selected voxels: about k % of the voxels carry one
    nz = int((g != 0).any(1).sum())
    N = int((target != 255.0).sum()) if mode == "oh" else g.shape[0] * g[0, 0].numel()
    assert nz <= k_count(N, k)


@pytest.mark.parametrize("mode,shape", [("oh", A), ("ml", B4)])
def test_k_100_is_the_cross_entropy(pkg, dev, mode, shape):
    """k = 100 selects every voxel: the loss is SegLoss(region="none", voxel="ce")'s voxel term, to 1e-5, and the reference's"""
    logits, target = inputs(shape, mode, None)
    _, ld, loss = run_case(pkg, dev, logits, target, 100.0, dict(mode_kw(mode)))
    t = pkg.SegLoss(region="none", voxel="ce", **mode_kw(mode)).terms(logits.to(dev), target.to(dev))
    assert relerr(loss, t[2]) < 1e-5


def test_k_small_enough_for_one_voxel(pkg, dev):
    logits, target = inputs(A, "oh", None)
    _, ld, loss = run_case(pkg, dev, logits, target, K_ONE, dict(ONEHOT))
    assert int((ld.grad != 0).any(1).sum()) == 1
    u, _ = voxel_values(logits, target)
    assert relerr(loss, u.max()) < 1e-5


def test_batch_scope(pkg, dev):
    """the K hardest voxels of the WHOLE batch: here all of them lie in item 1, and a per-item top-k gives another, known value"""
    logits, target = batch_scope_inputs()
    u, _ = voxel_values(logits, target)
    K = k_count(u.numel(), 10.0)
    assert torch.sort(u[1], descending=True).values[K - 1] > u[0].max()
    whole, per_item = topk_ref(logits, target, 10.0, **ONEHOT), topk_ref(logits, target, 10.0, per_item=True, **ONEHOT)
    assert abs(float(whole - per_item)) > 0.1 * float(whole)
    _, ld, loss = run_case(pkg, dev, logits, target, 10.0, dict(ONEHOT))
    assert not ld.grad[0].any() and ld.grad[1].any()
    assert relerr(loss, per_item) > 0.1


def test_ties_share_the_threshold_weight(pkg, dev):
    """K inside a group of bit-equal values: the loss and the gradient follow the symmetric rule, at the same bounds"""
    logits, target = tie_inputs()
    u, _ = voxel_values(logits, target)
    u = u.reshape(-1)
    k = 30.0
    K = k_count(u.numel(), k)
    t = torch.sort(u, descending=True).values[K - 1]
    n_gt, n_eq = int((u > t).sum()), int((u == t).sum())
    print(f"K {K} n_gt {n_gt} n_eq {n_eq}")
    assert n_eq > 100 and n_gt < K < n_gt + n_eq                       # the threshold cuts a group
    w = tie_weights(u, K)
    assert abs(float(w.sum()) - 1.0) < 1e-12 and len(set(w[u == t].tolist())) == 1
    X, grad = reference(logits, target, k, dict(ONEHOT))
    ld = logits.to(dev).requires_grad_(True)
    loss = pkg.TopKLoss(k=k, **ONEHOT)(ld, target.to(dev))
    (loss * UP).backward()
    e, eg = relerr(loss, X), relerr(ld.grad, grad)
    print(f"loss relerr {e:.3e} gradient relerr {eg:.3e}")
    assert e < 1e-5 and eg < 1e-4
    assert int((ld.grad != 0).any(1).sum()) == n_gt + n_eq             # every tied voxel carries gradient


def test_reproducible_run_to_run(pkg, dev):
    logits, target = inputs(C3, "oh", None)
    crit = pkg.TopKLoss(k=12.5, **ONEHOT)
    outs = []
    for _ in range(3):
        ld = logits.to(dev).requires_grad_(True)
        loss = crit(ld, target.to(dev))
        loss.backward()
        outs.append((loss.detach().clone(), ld.grad.clone()))
    assert all(torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]) for o in outs[1:])


@pytest.mark.parametrize("mode", ["oh", "ml"])
@pytest.mark.parametrize("shape,k", [(A, 12.5), (C3, 12.5)])
def test_inside_guard_with_poisoned_workspace(pkg, dev, mode, shape, k):
    """Inputs, outputs, the value buffer and the coefficients between NaN red zones, the scratch poisoned: a histogram word, a count
    or a partial sum that is read without having been written by this call, or a value or gradient element that is not written,
    reaches the result as a NaN or a wild count; a write past a buffer changes a red zone.  (1, 2, 17) runs the scalar loops with
    partial last blocks, (2, 3, 24) the 16-byte paths and seven select workgroups."""
    logits, target = inputs(shape, mode, None)
    poison_workspace(pkg.functional, dev)
    with Guard(dev) as gd:
        run_case(pkg, dev, logits, target, k, dict(mode_kw(mode)))
        torch.cuda.synchronize()
    assert gd.check() > 0


def test_unaligned_logits_take_the_scalar_loop(pkg, dev):
    """V % 4 == 0 but the logits start 4 bytes past a 16-byte boundary: the value pass must not issue 16-byte loads"""
    logits, target = inputs(B4, "oh", None)
    buf = torch.zeros(logits.numel() + 4, device=dev)
    ld = buf[1:1 + logits.numel()].view(logits.shape)
    ld.copy_(logits)
    assert ld.is_contiguous() and ld.data_ptr() % 16 == 4
    run_case(pkg, dev, logits, target, 10.0, dict(ONEHOT), ld=ld)


def test_set_k_is_read_by_the_next_call(pkg, dev):
    logits, target = inputs(B4, "oh", None)
    ld, td = logits.to(dev), target.to(dev)
    crit = pkg.TopKLoss(k=10.0, **ONEHOT)
    first = crit(ld, td)
    crit.set_k(25.0)
    second = crit(ld, td)
    assert torch.equal(second, pkg.TopKLoss(k=25.0, **ONEHOT)(ld, td)) and not torch.equal(second, first)
    with pytest.raises(ValueError, match="k="):
        crit.set_k(0.0)


def test_too_many_channels_is_unsupported(pkg, dev):
    logits = torch.zeros(1, 17, 4, 4, 4, device=dev)
    with pytest.raises(RuntimeError, match="unsupported"):
        pkg.TopKLoss(**ONEHOT)(logits, torch.zeros(1, 1, 4, 4, 4, device=dev))
    with pytest.raises(RuntimeError, match="unsupported"):
        pkg.DiceTopKLoss(**MULTI)(logits, torch.zeros(1, 17, 4, 4, 4, device=dev))


@pytest.mark.parametrize("mode", ["oh", "ml"])
def test_dice_topk_is_the_sum_of_its_terms(pkg, dev, mode):
    kw = mode_kw(mode)
    logits, target = inputs(C3, mode, None)
    td = target.to(dev)
    res = []
    for crit in (pkg.DiceTopKLoss(k=12.5, lambda_dice=0.7, lambda_topk=1.3, include_background=False, **kw),
                 lambda x, y: 0.7 * pkg.SegLoss(region="dice", voxel="none", include_background=False, **kw)(x, y)
                 + 1.3 * pkg.TopKLoss(k=12.5, **kw)(x, y)):
        ld = logits.to(dev).requires_grad_(True)
        loss = crit(ld, td)
        (loss * UP).backward()
        res.append((loss.detach(), ld.grad))
    assert relerr(res[0][0], res[1][0]) < 1e-5 and relerr(res[0][1], res[1][1]) < 1e-4
    # and against the references of the two terms
    from segloss_ref import segloss_ref
    z = logits.clone().requires_grad_(True)
    R, _ = segloss_ref(z, target, region="dice", voxel="none", include_background=False, **kw)
    X = 0.7 * R + 1.3 * topk_ref(z, target, k=12.5, **kw)
    (X * UP).backward()
    assert relerr(res[0][0], X.detach()) < 1e-5 and relerr(res[0][1], z.grad) < 1e-4


def test_captured_train_step_with_dice_topk(pkg, dev):
    """Three captured and three eager TrainStep steps with DiceTopKLoss on the geometry test_captured_train_step_with_dice_focal
    uses (C1, 32^3): finite losses, bit-equal losses and parameters.  Then set_k(50) between two replays: the next captured loss is
    the eager step's that was given k = 50 from the same state -- the captured kernels read k when they run."""
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
        crit = pkg.DiceTopKLoss(k=10.0, include_background=False, to_onehot_y=True, softmax=True)
        step = pkg.TrainStep(m, crit, opt, xd, yd, use_graph=mode == "graph", warmup=2)
        assert (step.graphs is not None) == (mode == "graph")
        losses = []
        for _ in range(3):
            step.run()
            losses.append(float(step.loss.detach()))
        torch.cuda.synchronize()
        params = flat["param"].clone()
        crit.set_k(50.0)
        step.run()
        losses.append(float(step.loss.detach()))
        torch.cuda.synchronize()
        res[mode] = (losses, params)
        flat["state"].clear()
        del step, opt, m, flat
    print("captured", res["graph"][0], "eager", res["eager"][0])
    assert all(l == l and abs(l) < float("inf") for l in res["graph"][0])
    assert res["graph"][0][:3] == res["eager"][0][:3]
    assert torch.equal(res["graph"][1], res["eager"][1])
    assert res["graph"][0][3] == res["eager"][0][3]
