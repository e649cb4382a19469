"""Gradient clipping, the parts that need no GPU: the host reference against torch.nn.utils.clip_grad_norm_ on CPU tensors, argument
validation of the optimizer option and the free function, the public surface."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import grad_clip_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("unetr_grad_sumsq_ranges", "unetr_grad_sumsq", "unetr_grad_clip_finalize", "unetr_grad_clip_set", "unetr_adamw_hyper_clip",
               "unetr_grad_scale_ranges", "unetr_grad_scale")


def _grads(seed, scale):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=gen) * scale for s in [(1,), (3, 5), (4097,), (2, 3, 4, 5, 7)]]


@pytest.mark.parametrize("scale", [1e-3, 1.0, 50.0])
@pytest.mark.parametrize("max_norm", [0.5, 12.0, float("inf")])
def test_reference_agrees_with_torch(scale, max_norm):
    """norm and scaled gradients of the float64 reference against torch.nn.utils.clip_grad_norm_ on CPU tensors: 1e-6 relative (torch
    sums in float32)"""
    grads = _grads(3, scale)
    params = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
    for p, g in zip(params, grads):
        p.grad = g.clone()
    total = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    norm, coef = R.clip_ref([g.numpy() for g in grads], max_norm)
    assert abs(float(norm) - total) <= 1e-6 * total
    assert (coef < 1.0) == (total + 1e-6 > max_norm)
    for p, g in zip(params, grads):
        want = g.numpy() * coef
        assert np.allclose(p.grad.numpy(), want, rtol=1e-6, atol=0.0)


def test_reference_edge_cases():
    big = np.full(16, 3e38, dtype=np.float32)
    n, c = R.clip_ref([big], 12.0)
    assert np.isinf(n) and c == 0.0
    n, c = R.clip_ref([np.array([1.0, np.nan], dtype=np.float32)], 12.0)
    assert np.isnan(n) and np.isnan(c)
    assert R.coef_f32(3.0, float("inf")) == 1.0 and R.coef_f32(12.0, 12.0) < 1.0 and R.coef_f32(1.0, 12.0) == 1.0
    assert np.isnan(R.coef_f32(float("inf"), float("inf")))
    assert R.norm_f32([np.array([3.0, 4.0], dtype=np.float32)], 1.0 / 3.0) == np.float32(np.float64(np.float32(1.0 / 3.0)) * 5.0)
    assert R.ulp_diff(1.0, np.nextafter(np.float32(1.0), np.float32(2.0))) == 1


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), float("-inf")])
def test_max_norm_validation(pkg, bad):
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError, match="max_norm"):
        pkg.AdamW([p], max_grad_norm=bad)
    opt = pkg.AdamW([p])
    with pytest.raises(ValueError, match="max_norm"):
        opt.set_max_grad_norm(bad)
    assert opt.max_grad_norm is None
    p.grad = torch.zeros(4)
    with pytest.raises(ValueError, match="max_norm"):
        pkg.clip_grad_norm_([p], bad)


@pytest.mark.parametrize("norm_type", [1, 1.0, float("inf"), 0.5])
def test_norm_type_validation(pkg, norm_type):
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.zeros(4)
    with pytest.raises(ValueError, match="norm_type"):
        pkg.clip_grad_norm_([p], 1.0, norm_type=norm_type)


def test_no_cpu_fallback(pkg):
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="ROCm device"):
        pkg.clip_grad_norm_([p], 1.0)
    with pytest.raises(ValueError, match="no parameter has a gradient"):
        pkg.clip_grad_norm_([torch.nn.Parameter(torch.zeros(4))], 1.0)


def test_option_is_off_by_default(pkg):
    p = torch.nn.Parameter(torch.zeros(4))
    opt = pkg.AdamW([p])
    assert opt.max_grad_norm is None and opt._clip is None
    with pytest.raises(RuntimeError, match="without max_grad_norm"):
        opt.grad_norm()
    assert "max_grad_norm" not in opt.state_dict()["param_groups"][0]
    assert pkg.AdamW([p], max_grad_norm=float("inf")).max_grad_norm == math.inf
    assert pkg.AdamW([p], max_grad_norm=12).max_grad_norm == 12.0
    opt.set_max_grad_norm(3)
    assert opt.max_grad_norm == 3.0
    opt.set_max_grad_norm(None)
    assert opt.max_grad_norm is None


def test_public_surface(pkg):
    assert pkg.clip_grad_norm_ is pkg.grad_clip.clip_grad_norm_ and "clip_grad_norm_" in pkg.__all__
    sig = inspect.signature(pkg.clip_grad_norm_).parameters
    assert list(sig) == ["parameters", "max_norm", "norm_type", "error_if_nonfinite"]
    assert sig["norm_type"].default == 2.0 and sig["error_if_nonfinite"].default is False
    assert inspect.signature(pkg.AdamW.__init__).parameters["max_grad_norm"].default is None
    assert inspect.signature(pkg.TrainStep.__init__).parameters["max_grad_norm"].default is None
    header = open(os.path.join(ROOT, "include", "unetr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for s in NEW_SYMBOLS:
        assert s in pkg._capi.EXPORTED_SYMBOLS, s
        assert re.search(r"\b%s\s*\(" % s, code), s
    # unetr_adamw_hyper_clip = unetr_adamw_hyper + one pointer before the stream
    a, b = pkg._capi._SIGNATURES["unetr_adamw_hyper"], pkg._capi._SIGNATURES["unetr_adamw_hyper_clip"]
    assert b == a[:-1] + [a[-1], a[-1]]
    assert pkg.grad_clip.BLOCK == 8192 and pkg.grad_clip.blocks_of(8193) == 2
