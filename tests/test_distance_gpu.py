"""The dense distance transform (csrc/edt.hip), its distance fields and the two distance-map losses (csrc/dist_loss.hip) against
the float64 / int64 references of tests/distance_ref.py.

Transform: the shapes of distance_ref.EDT_SHAPES -- listed there with the tile parameter each one sits next to (64 x per mask
word and 4 x-lines per block in the x pass; EDT_COLS = 32 columns and 8 rows per sweep in the column passes; EDT_TALL = 256 /
EDT_COLS_TALL = 16 for the z pass with two fields; the extent cap 512) -- times every mask kind, without and with the spacing
(3.0, 0.7, 1.5), one to three masks per call.  Bounds: squared distances without a spacing are exact integers, torch.equal;
everything else elementwise |a - b| <= 1e-6 * max(b, 1) and inf == inf: three non-negative terms with two roundings each and two
adds give at most 4 * 2^-24 relative on d^2, the square root halves that and adds one rounding, about 1.8e-7; the bound is about
5 x that (the float32 sqrt need not be correctly rounded).

Losses: shapes (B, C, S), V = S^3, those of test_segloss_gpu.py (forward chunk = 4096 voxels with 16-byte loads when V % 4 == 0,
backward block = 256 voxels): (1, 2, 17) odd V, scalar loop, two chunks; (2, 4, 16) one full chunk, 16-byte path; (2, 3, 24) several
chunks, the last partial; (1, 14, 12) the 14 classes of BTCV; (1, 1, 17) one channel, multilabel only.  Bounds: util.relerr < 1e-5
on the loss and < 1e-4 on the logits gradient, the project's bounds for this kernel family (test_ops_gpu.py::test_dicece,
test_segloss_gpu.py); a loss that is legitimately 0 (every field 0) by absolute error < 1e-6."""
import pytest
import torch

from distance_ref import (A, B4, C3, EDT_SHAPES, LOSS_CASES, MASK_KINDS, MULTI, ONEHOT, SPACING, edt_ref, fields_ref, loss_inputs,
                          loss_ref, make_mask)
from guard import Guard, poison_workspace
from util import relerr

pytestmark = pytest.mark.gpu

UP = 0.61      # the upstream gradient of every backward here


def edt_close(got, want):
    """the transform's bound, elementwise; inf == inf"""
    got, want = got.detach().double().cpu(), want.double()
    inf = torch.isinf(want)
    if not torch.equal(torch.isinf(got) & (got > 0), inf):
        return False
    g, w = got[~inf], want[~inf]
    return not torch.isnan(g).any() and bool(((g - w).abs() <= 1e-6 * w.abs().clamp_min(1.0)).all())


def check_edt(pkg, masks, spacing, arg):
    """masks: list of bool [D,H,W]; arg: the tensor handed to the package, whose volumes are the masks in order"""
    want2 = torch.stack([edt_ref(m, spacing, squared=True) for m in masks]).reshape(arg.shape)
    want = torch.stack([edt_ref(m, spacing) for m in masks]).reshape(arg.shape)
    got = pkg.distance_transform_edt(arg, spacing=spacing)
    got2 = pkg.distance_transform_edt(arg, spacing=spacing, squared=True)
    assert got.shape == arg.shape and got.dtype == torch.float32 and got2.shape == arg.shape
    assert edt_close(got, want)
    if spacing is None:
        assert torch.equal(got2.cpu(), want2.float())
    else:
        assert edt_close(got2, want2)


@pytest.mark.parametrize("spacing", [None, SPACING], ids=["unit", "aniso"])
@pytest.mark.parametrize("shape", EDT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edt(pkg, dev, shape, spacing):
    """every mask kind; one volume as float32 [*S], two as bool [N,*S], three as uint8 [1,3,*S], one as int64 [1,1,*S]"""
    m = {k: make_mask(k, shape) for k in MASK_KINDS}
    check_edt(pkg, [m["random"]], spacing, m["random"].float().to(dev))
    check_edt(pkg, [m["three_zeros"], m["corner_zero"]], spacing, torch.stack([m["three_zeros"], m["corner_zero"]]).to(dev))
    trio = [m["all_zeros"], m["no_zeros"], m["half_space"]]
    check_edt(pkg, trio, spacing, torch.stack(trio)[None].to(torch.uint8).to(dev))
    check_edt(pkg, [m["hollow_sphere"]], spacing, (m["hollow_sphere"].long() * 3)[None, None].to(dev))


@pytest.mark.parametrize("shape", [(5, 7, 9), (3, 70, 33), (257, 2, 3)], ids=lambda s: "x".join(map(str, s)))
def test_edt_inside_guard_with_poisoned_workspace(pkg, dev, shape):
    """inputs and outputs between NaN red zones, the scratch poisoned: a field element that is consumed without having been written
    or an output element that is not written is a NaN in the result, a write past a buffer changes a red zone"""
    masks = [make_mask(k, shape) for k in ("random", "half_space", "hollow_sphere")]
    poison_workspace(pkg.functional, dev)
    with Guard(dev) as gd:
        check_edt(pkg, masks, SPACING, torch.stack(masks).float().to(dev))
        objs = torch.stack(masks)[None]
        for unsigned in (False, True):
            got = pkg.signed_distance_map(objs.float().to(dev), unsigned=unsigned)
            assert edt_close(got, fields_ref(objs, None, unsigned))
        torch.cuda.synchronize()
    assert gd.check() > 0


def test_groups_when_the_workspace_is_small(pkg, dev, monkeypatch):
    """a scratch buffer that holds one item's two fields but not all three items': the items run one after the other, same result"""
    S = (6, 10, 12)
    objs = torch.stack([make_mask(k, S) for k in ("random", "half_space", "hollow_sphere")])[:, None]
    small = torch.empty(2 * 6 * 10 * 12 + 4, dtype=torch.float32, device=dev)
    full = pkg.signed_distance_map(objs.float().to(dev))
    monkeypatch.setattr(pkg.functional, "workspace", lambda device: small)
    assert torch.equal(pkg.signed_distance_map(objs.float().to(dev)), full)
    assert edt_close(full, fields_ref(objs))
    with pytest.raises(RuntimeError, match="workspace"):
        monkeypatch.setattr(pkg.functional, "workspace", lambda device: small[:100])
        pkg.signed_distance_map(objs.float().to(dev))


def test_three_input_forms_give_the_same_field(pkg, dev):
    """a float mask, class ids against the channel index, and logits thresholded inside the kernel (softmax and sigmoid)"""
    gen = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 3, (2, 1, 9, 12, 14), generator=gen)
    onehot = torch.zeros(2, 3, 9, 12, 14).scatter_(1, ids, 1.0)
    logits = (8.0 * (2.0 * onehot - 1.0) + torch.randn(onehot.shape, generator=gen)).to(dev)
    D = pkg.distance
    for sp in (None, SPACING):
        want = fields_ref(onehot, sp, unsigned=True)
        from_mask = pkg.signed_distance_map(onehot.to(dev), spacing=sp, unsigned=True)
        assert edt_close(from_mask, want)
        assert torch.equal(pkg.signed_distance_map(ids.float().to(dev), num_classes=3, spacing=sp, unsigned=True), from_mask)
        assert torch.equal(D.prediction_distance_map(logits, spacing=sp), from_mask)
        assert torch.equal(D.prediction_distance_map(logits, sigmoid=True, spacing=sp), from_mask)
        signed = pkg.signed_distance_map(onehot.to(dev), spacing=sp)
        assert torch.equal(pkg.signed_distance_map(ids.float().to(dev), num_classes=3, spacing=sp), signed)
        assert edt_close(signed, fields_ref(onehot, sp))
    # the plain transform of the same masks: the distance to the nearest zero is the field inside the object
    inside = pkg.distance_transform_edt(onehot.to(dev))
    obj = onehot.bool().to(dev)
    assert torch.equal(inside[obj], pkg.signed_distance_map(onehot.to(dev), unsigned=True)[obj])


def test_limits_raise_not_implemented(pkg, dev):
    for shape in ((1, 1, 513), (513, 1, 1), (1, 513, 1), (1, 17, 2, 2, 2)):
        with pytest.raises(NotImplementedError, match="up to 16 channels"):
            pkg.distance_transform_edt(torch.zeros(shape, device=dev))
    with pytest.raises(NotImplementedError):
        pkg.signed_distance_map(torch.zeros(1, 1, 2, 2, 2, device=dev), num_classes=17)
    logits = torch.zeros(1, 17, 4, 4, 4, device=dev)
    with pytest.raises(NotImplementedError):
        pkg.BoundaryLoss(**ONEHOT)(logits, torch.zeros(1, 1, 4, 4, 4, device=dev))
    with pytest.raises(NotImplementedError):
        pkg.HausdorffDTLoss(**MULTI)(logits, torch.zeros(1, 17, 4, 4, 4, device=dev))


@pytest.mark.parametrize("spacing", [None, SPACING], ids=["unit", "aniso"])
def test_fields_from_class_ids(pkg, dev, spacing):
    """(2, 3, 12^3): class 1 is absent from item 0 and item 1 is class 2 only -- those fields are 0, and nothing is NaN (inf - inf)"""
    gen = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 3, (2, 1, 12, 12, 12), generator=gen)
    ids[0][ids[0] == 1] = 0
    ids[1] = 2
    onehot = torch.zeros(2, 3, 12, 12, 12).scatter_(1, ids, 1.0)
    for unsigned in (False, True):
        got = pkg.signed_distance_map(ids.float().to(dev), num_classes=3, spacing=spacing, unsigned=unsigned)
        assert got.shape == onehot.shape and not torch.isnan(got).any() and not torch.isinf(got).any()
        assert edt_close(got, fields_ref(onehot, spacing, unsigned))
        assert not got[0, 1].any() and not got[1].any() and got[0, 0].any() and got[0, 2].any()


def test_fields_from_a_multilabel_mask(pkg, dev):
    gen = torch.Generator().manual_seed(4)
    mask = (torch.rand(1, 2, 17, 17, 17, generator=gen) < 0.35).float()
    for sp in (None, SPACING):
        for unsigned in (False, True):
            assert edt_close(pkg.signed_distance_map(mask.to(dev), spacing=sp, unsigned=unsigned), fields_ref(mask, sp, unsigned))


# ------------------------------------------------------------------------------------------------------------------- losses
ALL_BACKGROUND = ("bl-oh-A-all-background", "boundary", A, "oh", "background", "randn", dict())
_REF = {}


def case_inputs(case):
    _, _, shape, mode, label, logit, _ = case
    if label == "background":          # no object in any included channel: every field, the loss and the gradient are 0
        logits, _, _ = loss_inputs(shape, mode, "noise", logit)
        return logits, torch.zeros(shape[0], 1, shape[2], shape[2], shape[2])
    return loss_inputs(shape, mode, label, logit)[:2]


def reference(case):
    """(loss, gradient under the upstream gradient UP) in float64, computed once per case"""
    if case[0] not in _REF:
        logits, target = case_inputs(case)
        z = logits.double().requires_grad_(True)
        loss = loss_ref(case[1], z, target, case[3], case[6])
        (loss * UP).backward()
        _REF[case[0]] = (loss.detach(), z.grad)
    return _REF[case[0]]


def criterion(pkg, case):
    cls = pkg.BoundaryLoss if case[1] == "boundary" else pkg.HausdorffDTLoss
    return cls(**dict(ONEHOT if case[3] == "oh" else MULTI, **case[6]))


def run_case(pkg, dev, case, ld=None):
    logits, target = case_inputs(case)
    want, grad = reference(case)
    crit = criterion(pkg, case)
    if ld is None:
        ld = logits.to(dev)
    ld.requires_grad_(True)
    loss = crit(ld, target.to(dev))
    assert loss.dim() == 0
    (loss * UP).backward()
    loss = loss.detach()
    if case[4] == "background":
        assert abs(float(want)) < 1e-12 and abs(float(loss) - float(want)) < 1e-6
        e_loss = abs(float(loss))
    else:
        e_loss = relerr(loss, want)
    e_grad = relerr(ld.grad, grad)
    print(f"{case[0]}: loss {float(loss):.8g} reference {float(want):.8g} relerr {e_loss:.3e}, gradient relerr {e_grad:.3e}")
    assert e_loss < 1e-5 and e_grad < 1e-4
    return crit, loss, ld.grad


@pytest.mark.parametrize("case", LOSS_CASES + [ALL_BACKGROUND], ids=lambda c: c[0])
def test_loss_and_gradient(pkg, dev, case):
    _, kind, shape, mode, label, logit, opts = case
    logits, target = case_inputs(case)
    sp = opts.get("spacing")
    if label == "blob":                # the fields must reach deep: at least S / 3 voxels
        objs = target != 0 if mode == "ml" else torch.zeros(shape[0], shape[1], *target.shape[2:]).scatter_(1, target.long(), 1.0)
        assert float(fields_ref(objs, None, unsigned=True).max()) >= shape[2] / 3
    if kind == "hausdorff":            # outside the band the float32 and the float64 prediction masks are the same
        p = torch.sigmoid(logits.double()) if mode == "ml" else torch.softmax(logits.double(), 1)
        got = pkg.distance.prediction_distance_map(logits.to(dev), sigmoid=mode == "ml", spacing=sp)
        assert edt_close(got, fields_ref(p > 0.5, sp, unsigned=True))
    run_case(pkg, dev, case)


@pytest.mark.parametrize("case", [LOSS_CASES[1], LOSS_CASES[6], LOSS_CASES[12], LOSS_CASES[17]], ids=lambda c: c[0])
def test_loss_inside_guard_with_poisoned_workspace(pkg, dev, case):
    """(1, 2, 17) runs the forward's scalar loop with a partial second chunk and a partial last backward block, (2, 3, 24) the
    16-byte path with a partial last chunk; each under both losses"""
    poison_workspace(pkg.functional, dev)
    with Guard(dev) as gd:
        run_case(pkg, dev, case)
        torch.cuda.synchronize()
    assert gd.check() > 0


@pytest.mark.parametrize("case", [LOSS_CASES[3], LOSS_CASES[15]], ids=lambda c: c[0])
def test_unaligned_pointers_take_the_scalar_loop(pkg, dev, case):
    """V % 4 == 0 but the logits start 4 bytes past a 16-byte boundary: no 16-byte loads; the same result to the bounds"""
    logits, _ = case_inputs(case)
    res = []
    for shift in (0, 1):
        buf = torch.zeros(logits.numel() + 4, device=dev)
        ld = buf[shift:shift + logits.numel()].view(logits.shape)
        ld.copy_(logits)
        assert ld.is_contiguous() and ld.data_ptr() % 16 == 4 * shift
        _, loss, grad = run_case(pkg, dev, case, ld)
        res.append((loss, grad.clone()))
    assert relerr(res[1][0], res[0][0]) < 1e-5 and relerr(res[1][1], res[0][1]) < 1e-4


@pytest.mark.parametrize("case", [LOSS_CASES[5], LOSS_CASES[17]], ids=lambda c: c[0])
def test_reproducible_run_to_run(pkg, dev, case):
    outs = [run_case(pkg, dev, case)[1:] for _ in range(3)]
    assert all(torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]) for o in outs[1:])


@pytest.mark.parametrize("case", [LOSS_CASES[3], LOSS_CASES[11]], ids=lambda c: c[0])
def test_set_weight_under_capture(pkg, dev, case):
    """forward + backward captured on the side stream as TrainStep captures its step; set_weight between two replays re-weights
    the loss and the gradient: 0.25 times the first ones (weight 1), up to one rounding"""
    logits, target = case_inputs(case)
    crit = criterion(pkg, case)
    w0 = float(crit.weight)
    ld, td = logits.to(dev).requires_grad_(True), target.to(dev)
    side = pkg.train_step.side_stream(dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            ld.grad = None
            (crit(ld, td) * UP).backward()
    torch.cuda.current_stream().wait_stream(side)
    eager = ld.grad.clone()
    ld.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        loss = crit(ld, td)
        (loss * UP).backward()
    g.replay()
    torch.cuda.synchronize()
    l1, g1 = loss.detach().clone(), ld.grad.clone()
    assert torch.equal(g1, eager)
    crit.set_weight(0.25)
    g.replay()
    torch.cuda.synchronize()
    l2, g2 = loss.detach().clone(), ld.grad.clone()
    k = 0.25 / w0
    eps = 2.0 ** -23
    assert abs(float(l2) - k * float(l1)) <= eps * abs(k * float(l1))
    assert bool(((g2.double() - k * g1.double()).abs() <= eps * (k * g1.double()).abs()).all())
    assert float(l1) != 0.0 and g1.any()
    del g


def test_captured_train_step_with_dice_ce_plus_boundary(pkg, dev):
    """The distance-map losses compose with the others in plain torch inside TrainStep: three captured steps with
    SegLoss + BoundaryLoss on the smallest model geometry of test_model_gpu.py (C1, 32^3) give finite losses, the losses of three
    eager steps from the same state -- bit for bit, as test_segloss_gpu.py::test_captured_train_step_with_dice_focal holds them."""
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
        seg = pkg.SegLoss(include_background=False, to_onehot_y=True, softmax=True)
        bl = pkg.BoundaryLoss(to_onehot_y=True, softmax=True, weight=0.1)

        def crit(lg, t, seg=seg, bl=bl):
            return seg(lg, t) + bl(lg, t)

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
