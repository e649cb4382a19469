"""The kernel parity tests again, with the memory AROUND every operand under control (tests/guard.py).

Each case below calls the body of an existing GPU test -- its references, tolerances and assertions are used as they stand, nothing
is restated here -- after ``poison_workspace`` (the 256 MB ``functional.workspace`` holds the NaN pattern), inside ``Guard`` (every
input the body copies to the device and every ``torch.empty`` / ``new_empty`` / ``empty_like`` of the wrappers sits between two
64 KiB red zones, ``empty`` payloads hold the NaN pattern) and followed by ``check()`` (every red zone still holds its pattern
bit for bit).  A halo read off the end of a tensor, a partial-sum row that is consumed but never produced, a stale read of the
workspace or a ``0 * garbage`` then reaches the body's own comparison as NaN; a write past a ragged tail fails ``check()``.

Bodies that run guarded (shapes: the smallest / most ragged ones of each body's own list, every precision the body takes):
  test_ops_gpu: test_conv3, test_conv3_halo, test_conv3_fused_stats_and_1x1, test_conv3_dgrad_fused,
    test_conv3_dgrad_with_backward_statistics, test_conv3_wgrad_bf16x3_split_images, test_conv3_single_channel_image,
    test_resblock_in_fusion_levels, test_instnorm_finalize_in_apply_prologue, test_upblock_with_out_conv_head, test_tconv,
    test_instnorm, test_instnorm_bwd_folded_finalize, test_outconv_and_layout, test_reduce_rows_grouped, test_layernorm,
    test_gemm_ln_fwd_fused_equals_three_steps, test_gemm_ln_bwd_fused_equals_two_steps, test_colsum, test_attention,
    test_attention_bf16_storage, test_attention_bf16_forward_wave_counts, test_gemm_nt_nn_tn, test_gemm_bf16x3_dma,
    test_gemm_bf16_storage, test_gemm_bf16_small_m_tiles, test_gemm_epilogues, test_gemm_bf16_epilogues,
    test_gemm_bf16_grouped_wgrad, test_grouped_wgrad_fused_epilogues, test_patch_embed, test_dicece,
    test_dicece_sigmoid_multilabel, test_adamw, test_ranking_losses; and, beyond the issue's lists, test_gemm_bf16_big_tile (forced
    onto ragged shapes), test_gemm_padding_lanes_ignore_inf_nan, test_tr16_probe, test_ranking_losses_vs_reference_fixture
  test_lr_schedule_gpu: test_adamw_hyper_equals_by_value, test_arena_hyper_equals_by_value, test_counter_add_lr
  test_wt_shadow_gpu: test_transpose_grouped_derive_launch, test_fused_epilogue_writes_transposed_shadow
  test_prefetch_rider_gpu: test_layernorm_fwd_rider, test_layernorm_bwd_rider, test_layernorm_fwd_slab_form_rider,
    test_layernorm_bwd_slab_form_rider, test_attention_bf16_rider
  test_inference_gpu: test_gather_batch_equals_pad_and_slice, test_accumulate_batch_equals_sequential_accumulate,
    test_finalize_post_forms
  test_metrics_gpu: test_hd_exact_on_organs (its smallest volume), test_hd_edge_cases_and_options
  test_postprocess_gpu: test_random_masks_against_scipy (its smallest shape), test_long_equivalence_chains_across_workgroups
  test_augment_gpu: test_index_lists_exact, test_apply_explicit_tables
  test_preprocess_gpu: test_border_clamping_at_all_six_faces, test_identity_spacing_is_a_bit_exact_flip_transpose
(The three "conv3 fusion" bodies take different parameters: the up-block body runs (2,5,16,3) and (1,6,16,2); the residual-block and
finalize-in-prologue bodies run the image case on the ragged (9,7,19) volume and the smallest many-channel case of their own lists.)

Left out: every body that captures a hipGraph (a guarded allocation during capture is not what this file tests), every body that
spawns processes, the model-level tests, and test_skip_written_into_concat_buffer (functional.cat_of_skip identifies the
concatenation buffer by its storage, which a guarded tensor shares with its red zones).  No body of the lists above is left out.

Backward passes: torch runs ``autograd.Function.backward`` of GPU nodes on a device worker thread, and hands that thread the
dispatch-mode stack of the thread that called ``.backward()``: the mode IS active there, the allocations of the backward wrappers
are guarded like the forward ones (test_backward_allocations_are_guarded counts them), nothing is called separately.

test_pitched_operands_in_poisoned_concat_halves is the one body of its own: the direct wrappers that take a row pitch, fed from /
writing into one half of a 2C-wide buffer whose other half holds the pattern.
"""
import inspect
import itertools

import pytest
import torch

import test_augment_gpu as t_aug
import test_inference_gpu as t_inf
import test_lr_schedule_gpu as t_lr
import test_metrics_gpu as t_met
import test_ops_gpu as ops
import test_postprocess_gpu as t_post
import test_prefetch_rider_gpu as t_pf
import test_preprocess_gpu as t_pre
import test_wt_shadow_gpu as t_wt
from guard import Guard, holds_pattern, poison_workspace, poisoned

pytestmark = pytest.mark.gpu

P3, P2 = [0, 1, 2], [0, 1]


def listed(fn):
    """the cases the body's own file lists: the product of its parametrize marks"""
    axes = []
    for m in getattr(fn, "pytestmark", []):
        if m.name != "parametrize":
            continue
        names = [n.strip() for n in m.args[0].split(",")] if isinstance(m.args[0], str) else list(m.args[0])
        axes.append([dict(zip(names, v if len(names) > 1 else (v,))) for v in m.args[1]])
    return [{k: v for d in combo for k, v in d.items()} for combo in itertools.product(*axes)]


def rows(names, values, **axes):
    """explicit cases: `values` under `names`, times every further axis"""
    names = names.split(",")
    out = [dict(zip(names, v if len(names) > 1 else (v,))) for v in values]
    for k, vs in axes.items():
        out = [dict(c, **{k: v}) for c in out for v in vs]
    return out


def only(fn, **keep):
    """the listed cases whose parameters are among `keep`"""
    return [c for c in listed(fn) if all(c[k] in v for k, v in keep.items())]


CONV3 = [(1, (5, 6, 7), 8, 16), (1, (6, 5, 4), 4, 16), (1, (4, 4, 4), 64, 32)]
DGRAD = [(1, (9, 7, 19), 16, 16), (1, (5, 6, 7), 16, 32)]

GUARDED = [
    # ---- test_ops_gpu
    (ops.test_conv3, rows("B,dims3,cin,cout", CONV3, prec=P3)),
    (ops.test_conv3_halo, rows("B,dims3,cin,cout", CONV3, prec=P3)),
    (ops.test_conv3_fused_stats_and_1x1, rows("B,dims3,cin,cout,with3", [(1, (9, 7, 19), 1, 16, True), (1, (5, 6, 7), 16, 32, False),
                                                                         (2, (4, 4, 16), 256, 128, True)], prec=P3)),
    (ops.test_conv3_dgrad_fused, rows("B,dims3,cin,cout", DGRAD, prec=P3)),
    (ops.test_conv3_dgrad_with_backward_statistics, rows("B,dims3,C,cout", DGRAD, max_wg=[0], prec=P3)),
    (ops.test_conv3_wgrad_bf16x3_split_images, only(ops.test_conv3_wgrad_bf16x3_split_images, dims3=[(9, 7, 19)])),
    (ops.test_conv3_single_channel_image, rows("B,dims3,max_wg", [(2, (9, 7, 19), 0)])),
    (ops.test_resblock_in_fusion_levels, rows("B,dims3,cin,cout", [(3, (9, 7, 19), 1, 16), (2, (6, 6, 6), 256, 128)], prec=P3)),
    (ops.test_instnorm_finalize_in_apply_prologue, rows("B,dims3,cin,cout,with3", [(1, (9, 7, 19), 1, 16, True), (2, (4, 4, 16), 256, 128, True)],
                                                        prec=P2)),
    (ops.test_upblock_with_out_conv_head, rows("B,S,C,ncls", [(2, 5, 16, 3), (1, 6, 16, 2)], prec=P3)),
    (ops.test_tconv, rows("B,S,cin,cout", [(1, 5, 32, 16), (1, 17, 16, 8), (1, 13, 64, 32), (2, 6, 768, 32)], prec=P3)),
    (ops.test_instnorm, rows("B,S,C", [(2, 6, 128), (1, 20, 32)], prec=P2)),
    (ops.test_instnorm_bwd_folded_finalize, rows("B,S,C", [(2, 6, 128), (1, 20, 32)], prec=P2)),
    (ops.test_outconv_and_layout, listed(ops.test_outconv_and_layout)),
    (ops.test_reduce_rows_grouped, rows("n,G", [(35, 9), (16, 300)])),
    (ops.test_layernorm, rows("M,H", [(19, 772), (33, 1024), (8, 128)])),
    (ops.test_gemm_ln_fwd_fused_equals_three_steps, rows("M,N,K", [(64, 128, 256)])),
    (ops.test_gemm_ln_bwd_fused_equals_two_steps, rows("M,N,K", [(64, 128, 256)])),
    (ops.test_colsum, [{}]),
    (ops.test_attention, rows("B,L,heads,dh", [(1, 33, 2, 32), (1, 8, 4, 32), (2, 100, 3, 128)], prec=P3)),
    (ops.test_attention_bf16_storage, rows("B,L,heads", [(1, 8, 2), (3, 230, 1)])),
    (ops.test_attention_bf16_forward_wave_counts, rows("B,L,heads", [(1, 40, 2)], nw=[2, 4, 8])),
    (ops.test_gemm_nt_nn_tn, rows("M,N,K", [(37, 50, 44), (1000, 16, 32)], prec=P3)),
    (ops.test_gemm_bf16x3_dma, rows("M,N,K", [(430, 772, 96), (33, 64, 32)])),
    (ops.test_gemm_bf16_storage, rows("M,N,K", [(37, 56, 64)])),
    (ops.test_gemm_bf16_small_m_tiles, listed(ops.test_gemm_bf16_small_m_tiles)),
    (ops.test_gemm_epilogues, listed(ops.test_gemm_epilogues)),
    (ops.test_gemm_bf16_epilogues, [{}]),
    (ops.test_gemm_bf16_grouped_wgrad, [{}]),
    (ops.test_grouped_wgrad_fused_epilogues, [{}]),
    (ops.test_patch_embed, [{}]),
    (ops.test_dicece, rows("B,C,S", [(1, 2, 17)])),
    (ops.test_dicece_sigmoid_multilabel, rows("B,C,S", [(1, 4, 17)])),
    (ops.test_adamw, [{}]),
    (ops.test_ranking_losses, rows("shape,slice_dim,init_idx", [((4, 3, 16, 8, 24), 3, 1)], kind=["ranking", "contrastive"])),
    # (beyond the issue's lists: the 256-row tiles forced onto ragged M / N tails, the clamped padding lanes, two small fixtures)
    (ops.test_gemm_bf16_big_tile, rows("M,N,K,force", [(1030, 520, 192, 4), (1030, 520, 192, 3), (1300, 130, 256, 2)])),
    (ops.test_gemm_padding_lanes_ignore_inf_nan, rows("M,N,K", [(37, 50, 44), (70, 33, 4100)], prec=P3)),
    (ops.test_tr16_probe, [{}]),
    (ops.test_ranking_losses_vs_reference_fixture, [{}]),
    # ---- the other GPU test files
    (t_lr.test_adamw_hyper_equals_by_value, listed(t_lr.test_adamw_hyper_equals_by_value)),
    (t_lr.test_arena_hyper_equals_by_value, listed(t_lr.test_arena_hyper_equals_by_value)),
    (t_lr.test_counter_add_lr, listed(t_lr.test_counter_add_lr)),
    (t_wt.test_transpose_grouped_derive_launch, [{}]),
    (t_wt.test_fused_epilogue_writes_transposed_shadow, [{}]),
    (t_pf.test_layernorm_fwd_rider, listed(t_pf.test_layernorm_fwd_rider)),
    (t_pf.test_layernorm_bwd_rider, listed(t_pf.test_layernorm_bwd_rider)),
    (t_pf.test_layernorm_fwd_slab_form_rider, listed(t_pf.test_layernorm_fwd_slab_form_rider)),
    (t_pf.test_layernorm_bwd_slab_form_rider, listed(t_pf.test_layernorm_bwd_slab_form_rider)),
    (t_pf.test_attention_bf16_rider, listed(t_pf.test_attention_bf16_rider)),
    (t_inf.test_gather_batch_equals_pad_and_slice, listed(t_inf.test_gather_batch_equals_pad_and_slice)),
    (t_inf.test_accumulate_batch_equals_sequential_accumulate, listed(t_inf.test_accumulate_batch_equals_sequential_accumulate)),
    (t_inf.test_finalize_post_forms, listed(t_inf.test_finalize_post_forms)),
    (t_met.test_hd_exact_on_organs, rows("B,C,shape", [(1, 3, (91, 109, 91))])),
    (t_met.test_hd_edge_cases_and_options, [{}]),
    (t_post.test_random_masks_against_scipy, only(t_post.test_random_masks_against_scipy, shape=[(1, 1, 5, 7, 67)])),
    (t_post.test_long_equivalence_chains_across_workgroups, listed(t_post.test_long_equivalence_chains_across_workgroups)),
    (t_aug.test_index_lists_exact, listed(t_aug.test_index_lists_exact)),
    (t_aug.test_apply_explicit_tables, listed(t_aug.test_apply_explicit_tables)),
    (t_pre.test_border_clamping_at_all_six_faces, listed(t_pre.test_border_clamping_at_all_six_faces)),
    (t_pre.test_identity_spacing_is_a_bit_exact_flip_transpose, listed(t_pre.test_identity_spacing_is_a_bit_exact_flip_transpose)),
]


def _short(v):
    if isinstance(v, dict):
        return "+".join(f"{k}{_short(x)}" for k, x in v.items()) or "-"
    if isinstance(v, (tuple, list)):
        return "x".join(_short(x) for x in v)
    return str(v)


def _params():
    out = []
    for body, cases in GUARDED:
        assert cases, body.__name__                     # a filter that matches nothing must not pass silently
        want = set(inspect.signature(body).parameters) - {"pkg", "dev", "monkeypatch"}
        for case in cases:
            assert set(case) == want, (body.__name__, sorted(case), sorted(want))
            tag = "-".join(_short(v) for v in case.values())
            out.append(pytest.param(body, case, id=f"{body.__module__[5:-4]}.{body.__name__[5:]}" + (f"[{tag}]" if tag else "")))
    return out


@pytest.mark.parametrize("body,case", _params())
def test_guarded(pkg, dev, monkeypatch, body, case):
    if "monkeypatch" in inspect.signature(body).parameters:
        case = dict(case, monkeypatch=monkeypatch)
    poison_workspace(pkg.functional, dev)
    with Guard(dev) as gd:
        body(pkg=pkg, dev=dev, **case)
    assert gd.check() > 0


def test_guard_on_the_device(pkg, dev):
    """what tests/test_guard_cpu.py proves on CPU tensors holds for device memory: layout, alignment, poisoned payloads, inputs
    whose red zones hold the pattern, the poisoned workspace -- and nothing here writes out of bounds"""
    Fn = pkg.functional
    ws = poison_workspace(Fn, dev)
    assert holds_pattern(ws[:4096]) and holds_pattern(ws[-4096:]) and holds_pattern(ws[ws.numel() // 2::65537])
    x = ops.g(3, 5, 7, seed=1)
    with Guard(dev) as gd:
        xd = x.to(dev)
        xb = xd.bfloat16()
        xc = xd.permute(2, 0, 1).contiguous()
        e32, e16 = torch.empty(37, 3, device=dev), xb.new_empty(11)
        ei, el = torch.empty(9, dtype=torch.int32, device=dev), torch.empty_like(xd)
        z = torch.zeros(5, device=dev)
    assert len(gd.records) == 8
    assert torch.equal(xd.cpu(), x) and torch.equal(xb.cpu(), x.bfloat16()) and torch.equal(xc.cpu(), x.permute(2, 0, 1)) and not z.any()
    for t in (xd, xb, xc, e32, e16, ei, el, z):
        assert t.data_ptr() % 256 == 0 and t.is_contiguous()
    for t in (e32, e16, ei, el):
        assert holds_pattern(t)
    assert e32.isnan().all() and e16.isnan().all() and (ei == 0x5A5A5A5A).all()
    for rec in gd.records:
        for _, zone in rec.zones():
            assert zone.numel() * rec.dtype.itemsize >= 65536
    assert gd.check() == 8


def test_backward_allocations_are_guarded(pkg, dev):
    """The mode is active inside autograd.Function.backward although the engine runs it on a device worker thread: OutConvFn's
    backward allocates its three gradients through the wrappers, and all of them are recorded."""
    Fn = pkg.functional
    x = ops.g(2, 5, 6, 7, 16, seed=1)
    w, b, dl = ops.g(3, 16, 1, 1, 1, seed=2), ops.g(3, seed=3), ops.g(2, 3, 5, 6, 7, seed=4)
    with Guard(dev) as gd:
        xd, wd, bd = (t.to(dev).requires_grad_(True) for t in (x, w, b))
        y = Fn.OutConvFn.apply(xd, wd, bd)
        dld = dl.to(dev)
        torch.cuda.synchronize()
        before = len(gd.records)
        y.backward(dld)
        torch.cuda.synchronize()
        during = len(gd.records) - before
    print(f"guarded allocations: {before} before .backward(), {during} inside it")
    assert before >= 5 and during >= 3
    assert xd.grad is not None and wd.grad is not None and bd.grad is not None
    gd.check()


# ------------------------------------------------------------------------------------------ pitched operands in concat halves
def _first_half(t, dev):
    """t [..., C] as the first half of a [..., 2C] buffer whose second half holds the pattern: (buffer, view)"""
    C = t.shape[-1]
    buf = poisoned((*t.shape[:-1], 2 * C), t.dtype, dev)
    buf[..., :C] = t.to(dev)
    return buf, buf[..., :C]


def _second_half(shape, dtype, dev):
    """an output [..., C] as the second half of a [..., 2C] buffer that holds the pattern everywhere: (buffer, view)"""
    C = shape[-1]
    buf = poisoned((*shape[:-1], 2 * C), dtype, dev)
    return buf, buf[..., C:]


def _same_bits(a, b):
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b)
        for s, t in zip(a, b):
            _same_bits(s, t)
    elif a is None or not isinstance(a, torch.Tensor):
        assert a == b
    else:
        assert a.dtype == b.dtype and a.shape == b.shape
        ia = a.contiguous().view({2: torch.int16, 4: torch.int32}[a.dtype.itemsize])
        assert torch.equal(ia, b.contiguous().view(ia.dtype))
        assert not torch.isnan(a.float()).any()


@pytest.mark.parametrize("prec", P2)
@pytest.mark.parametrize("wrapper", ["conv3", "conv3_fused", "conv3_parts", "conv3_wgrad", "instnorm_stats", "instnorm_apply", "instnorm_bwd",
                                     "tconv_bwd", "tconv_dgrad", "tconv_wgrad", "unetr_copy_rows"])
def test_pitched_operands_in_poisoned_concat_halves(pkg, dev, wrapper, prec):
    """Every direct wrapper that takes a row pitch (ldx / lddy / ldo), at one ragged shape: each pitched input is the first half and
    each pitched output the second half of a 2C-wide buffer that holds the NaN pattern elsewhere.  The results are the dense call's
    bit for bit, and the halves the call must not touch still hold the pattern bit for bit.  (conv3_dgrad_fused, outconv_in_fwd and
    outconv_in_bwd pass the channel count as every pitch: there is nothing to place; the block tests cover their callers.)"""
    Fn = pkg.functional
    adt = Fn.act_dtype(prec)
    B, D, H, W = dims = (2, 5, 6, 7)
    V = D * H * W
    cin, cout = 16, 32
    fm = lambda *shape, seed: ops.act(ops.g(*shape, seed=seed), prec, dev)          # a feature map in the storage type of `prec`
    x, dy = fm(B, D, H, W, cin, seed=1), fm(B, D, H, W, cout, seed=2)
    w, w3 = ops.g(cout, cin, 3, 3, 3, seed=3, scale=0.2).to(dev), ops.g(cout, cin, 1, 1, 1, seed=4, scale=0.5).to(dev)
    xbuf, xv = _first_half(x, dev)
    dybuf, dyv = _first_half(dy, dev)
    poison_workspace(Fn, dev)
    untouched = [xbuf[..., cin:], dybuf[..., cout:]]
    with Guard(dev) as gd:
        if wrapper == "conv3":
            obuf, ov = _second_half((B, D, H, W, cout), adt, dev)
            Fn.conv3(xv, 2 * cin, w, dims, prec, out=ov, ldo=2 * cout)
            _same_bits(ov, Fn.conv3(x, cin, w, dims, prec))
            dbuf, dv = _second_half((B, D, H, W, cin), adt, dev)                   # and the data-gradient form
            Fn.conv3(dyv, 2 * cout, w, dims, prec, mode=1, out=dv, ldo=2 * cin)
            _same_bits(dv, Fn.conv3(dy, cout, w, dims, prec, mode=1))
            untouched += [obuf[..., :cout], dbuf[..., :cin]]
        elif wrapper == "conv3_fused":
            _same_bits(Fn.conv3_fused(xv, 2 * cin, w, w3, dims, prec), Fn.conv3_fused(x, cin, w, w3, dims, prec))
        elif wrapper == "conv3_parts":
            got, ref = Fn.conv3_parts(xv, 2 * cin, w, w3, dims, prec), Fn.conv3_parts(x, cin, w, w3, dims, prec)
            assert got is not None and got[4] == ref[4] and 0 < got[4] <= Fn.CONV3_MAX_ROWS
            used = lambda part: part.flatten()[:B * got[4] * 2 * cout]      # the kernels lay the rows out as part[B][rows][2][Cout]
            _same_bits((got[0], used(got[1]), got[2], used(got[3])), (ref[0], used(ref[1]), ref[2], used(ref[3])))
        elif wrapper == "conv3_wgrad":
            dy3 = fm(B, D, H, W, cout, seed=5)
            o3a, o3b = torch.empty(cout, cin, 1, 1, 1, device=dev), torch.empty(cout, cin, 1, 1, 1, device=dev)
            _same_bits(Fn.conv3_wgrad(xv, 2 * cin, dyv, 2 * cout, dims, cin, cout, prec, dy3=dy3, out3=o3a),
                       Fn.conv3_wgrad(x, cin, dy, cout, dims, cin, cout, prec, dy3=dy3, out3=o3b))
            _same_bits(o3a, o3b)
        elif wrapper == "instnorm_stats":
            _same_bits(Fn.instnorm_stats(xv, 2 * cin, B, V, cin), Fn.instnorm_stats(x, cin, B, V, cin))
        elif wrapper == "instnorm_apply":
            sa, x2 = Fn.instnorm_stats(x, cin, B, V, cin), fm(B, D, H, W, cin, seed=6)
            sb = Fn.instnorm_stats(x2, cin, B, V, cin)
            for kw in (dict(), dict(x2=x2, sb=sb)):
                obuf, ov = _second_half((B, D, H, W, cin), adt, dev)
                Fn.instnorm_apply(x, sa, B, V, cin, True, out=ov, ldo=2 * cin, **kw)
                _same_bits(ov, Fn.instnorm_apply(x, sa, B, V, cin, True, **kw))
                untouched.append(obuf[..., :cin])
        elif wrapper == "instnorm_bwd":
            c, c2 = fm(B, D, H, W, cout, seed=6), fm(B, D, H, W, cout, seed=7)
            sa, sb = Fn.instnorm_stats(c, cout, B, V, cout), Fn.instnorm_stats(c2, cout, B, V, cout)
            for kw in (dict(), dict(x2=c2, sb=sb)):
                _same_bits(Fn.instnorm_bwd(dyv, 2 * cout, c, sa, B, V, cout, True, **kw), Fn.instnorm_bwd(dy, cout, c, sa, B, V, cout, True, **kw))
        elif wrapper.startswith("tconv"):
            # 13^3 voxels, 16 -> 8 channels: the dedicated transposed-conv kernels (test_tconv); 5 x 6 x 7 voxels: the generic family
            for tdims, ci, co in (((1, 13, 13, 13), 16, 8), (dims, cin, cout)):
                tb, td, th, tw_ = tdims
                tx, tdy = fm(*tdims, ci, seed=8), fm(tb, 2 * td, 2 * th, 2 * tw_, co, seed=9)
                wt = ops.g(ci, co, 2, 2, 2, seed=10, scale=0.1).to(dev)
                (txbuf, txv), (tdbuf, tdv) = _first_half(tx, dev), _first_half(tdy, dev)
                if wrapper == "tconv_bwd":
                    _same_bits(Fn.tconv_bwd(txv, 2 * ci, None, tdv, 2 * co, wt, tdims, ci, co, prec, True),
                               Fn.tconv_bwd(tx, ci, None, tdy, co, wt, tdims, ci, co, prec, True))
                elif wrapper == "tconv_dgrad":
                    _same_bits(Fn.tconv_dgrad(tdv, 2 * co, wt, tdims, ci, co, prec), Fn.tconv_dgrad(tdy, co, wt, tdims, ci, co, prec))
                else:
                    _same_bits(Fn.tconv_wgrad(txv, 2 * ci, tdv, 2 * co, tdims, ci, co, prec), Fn.tconv_wgrad(tx, ci, tdy, co, tdims, ci, co, prec))
                untouched += [txbuf[..., ci:], tdbuf[..., co:]]
        else:
            st = torch.cuda.current_stream().cuda_stream
            for accumulate in (0, 1):
                obuf, ov = _second_half((B, D, H, W, cin), adt, dev)
                ov.copy_(x * 2)
                pkg._capi.call("unetr_copy_rows", ov.data_ptr(), 2 * cin, xv.data_ptr(), 2 * cin, B * V, cin, accumulate, int(prec == 1), st)
                _same_bits(ov, x * 3 if accumulate else x)
                untouched.append(obuf[..., :cin])
    gd.check()
    for k, t in enumerate(untouched):
        assert holds_pattern(t), k
