"""Host side of the learning-rate schedules: ``optim.schedule_lr`` -- the formula the step-counter launch evaluates on the device
(include/unetr_hip.h: unetr_lr_schedule), in Python floats rounded once to float32 -- at points that can be derived by hand, and the
argument checks of ``AdamW.set_schedule``.  No GPU."""
import struct

import pytest
import torch


def f32(x):
    return struct.unpack("f", struct.pack("f", float(x)))[0]


def sched(kind, base=1e-3, warmup=0, total=0, power=0.9, min_lr=0.0):
    return dict(kind=kind, base_lr=base, warmup=warmup, total=total, power=power, min_lr=min_lr)


def test_warmup_cosine_points(pkg):
    lr = pkg.optim.schedule_lr
    base = 1e-3
    s = sched("warmup_cosine", base, warmup=2, total=6)
    assert lr(s, 0) == 0.0                          # the first step uses f(0), as torch's schedulers do
    assert lr(s, 1) == f32(f32(base) * 0.5)         # linear warm-up: 1 / 2
    assert lr(s, 2) == f32(base)                    # cos(0) = 1
    assert lr(s, 4) == f32(f32(base) * 0.5)         # half way down: 0.5 (1 + cos(pi / 2)), cos(pi / 2) = 6e-17 vanishes next to 1
    assert lr(s, 6) == 0.0 and lr(s, 7) == 0.0 and lr(s, 1000) == 0.0
    s = sched("warmup_cosine", base, warmup=2, total=6, min_lr=1e-5)
    assert lr(s, 6) == f32(1e-5) and lr(s, 50) == f32(1e-5)
    assert lr(s, 0) == f32(1e-5)                    # the floor holds during warm-up as well
    assert lr(s, 2) == f32(base)
    # monotone down after the warm-up
    vals = [lr(sched("warmup_cosine", base, warmup=3, total=40), k) for k in range(3, 41)]
    assert all(a >= b for a, b in zip(vals[:-1], vals[1:])) and vals[0] == f32(base) and vals[-1] == 0.0


def test_poly_points(pkg):
    lr = pkg.optim.schedule_lr
    base = 1e-2
    s = sched("poly", base, total=4, power=2.0)
    assert lr(s, 0) == f32(base)
    assert lr(s, 2) == f32(f32(base) * 0.25)        # (1 - 2/4)^2
    assert lr(s, 4) == 0.0 and lr(s, 9) == 0.0      # s is clamped at total
    s = sched("poly", base, total=4, power=2.0, min_lr=5e-3)
    assert lr(s, 2) == f32(5e-3) and lr(s, 1) == f32(f32(base) * 0.5625)


def test_constant_and_floor(pkg):
    lr = pkg.optim.schedule_lr
    s = sched("constant", 3e-4)
    assert [lr(s, k) for k in (0, 1, 17, 10 ** 6)] == [f32(3e-4)] * 4
    assert lr(sched("constant", 3e-4, min_lr=1e-3), 5) == f32(1e-3)
    assert isinstance(lr(s, 0), float)


def test_set_schedule_arguments(pkg):
    p = torch.nn.Parameter(torch.zeros(4))
    opt = pkg.AdamW([p], lr=1e-3)
    with pytest.raises(ValueError, match="unknown schedule"):
        opt.set_schedule("exponential", total=5)
    with pytest.raises(ValueError, match="total"):
        opt.set_schedule("warmup_cosine", warmup=2)
    with pytest.raises(ValueError, match="invalid schedule"):
        opt.set_schedule("poly", total=0)
    with pytest.raises(ValueError, match="invalid schedule"):
        opt.set_schedule("warmup_cosine", warmup=-1, total=5)
    assert opt.schedule_lr(3) == f32(1e-3)          # no schedule attached: the group's rate
    opt.set_schedule("warmup_cosine", warmup=2, total=6, min_lr=1e-6)
    assert opt.schedule_lr(2) == f32(1e-3) and opt.schedule_lr(6) == f32(1e-6)
    opt.param_groups[0]["lr"] = 5.0                 # with a schedule attached the group's lr is no longer read: base_lr was taken at the call
    assert opt.schedule_lr(2) == f32(1e-3)
    # the checkpoint schema carries the description and the step count, next to what torch.optim.AdamW needs to load the group
    g = opt.state_dict()["param_groups"][0]
    assert g["schedule"] == dict(kind="warmup_cosine", warmup=2, total=6, power=0.9, min_lr=1e-6, base_lr=1e-3)
    assert g["t"] == 0 and g["decoupled_weight_decay"] is True and g["amsgrad"] is False and g["params"] == [0]
    assert opt.state_dict()["state"] == {}
