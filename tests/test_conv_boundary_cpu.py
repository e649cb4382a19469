"""The two casts between activation storage and the fp32-only generic kernel families (functional._f32_rows / _act_rows) on CPU
tensors.  tests/test_conv_routes_cpu.py pins where they are used; their results appear there only as `other`."""
import torch


def test_generic_family_boundary_casts(pkg):
    """what the log shows as `other`: the fp32 rows handed to the generic family hold exactly the values of the first c channels, and the
    way back is the storage type's own rounding, into a new tensor or into the half of a wider buffer"""
    Fn = pkg.functional
    torch.manual_seed(0)
    wide = torch.randn(2, 3, 8).to(torch.bfloat16)
    for t, ld in ((wide, 8), (wide[..., :4], 8), (wide[..., 4:], 8)):
        c = 8 if t is wide else 4
        r, pitch = Fn._f32_rows(t, ld, c)
        assert r.dtype == torch.float32 and r.is_contiguous() and pitch == c == r.stride(-2) and torch.equal(r, t[..., :c].float())
    r, pitch = Fn._f32_rows(wide, 8, 4)                  # a whole buffer named with the pitch of its rows: the first c channels
    assert pitch == 4 and torch.equal(r, wide[..., :4].float())
    f = torch.randn(2, 3, 8)
    half = f[..., 4:]
    r, pitch = Fn._f32_rows(half, 8, 4)                  # fp32: the tensor itself
    assert r is half and pitch == 8
    x32 = torch.randn(2, 3, 4)
    assert Fn._act_rows(x32, 0) is x32 and Fn._act_rows(x32, 2) is x32
    assert torch.equal(Fn._act_rows(x32, 1), x32.to(torch.bfloat16))
    cat = torch.zeros(2, 3, 8, dtype=torch.bfloat16)
    assert Fn._act_rows(x32, 1, out=cat[..., 4:]).data_ptr() == cat[..., 4:].data_ptr()
    assert torch.equal(cat[..., 4:], x32.to(torch.bfloat16)) and not cat[..., :4].any()
