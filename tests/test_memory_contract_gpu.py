"""Memory contract of the HIP entry points: the existing float64-oracle parity cases re-run with every output, workspace and partial
buffer poisoned (NaN, followed by a guard band: tests/memcheck.py), plus the checks that poison alone cannot reach -- inputs left
bit-identical, channel-slice views with NaN in the gap, capacities at exactly the queried size and one block less, and a second call
on the first call's leftover workspace.  A read-before-write shows up as NaN in the parity check, a tail write as a broken guard."""
import math

import pytest
import torch

import memcheck as M
import test_bf16_storage_gpu as BF
import test_dwmarch_gpu as DM
import test_ops_gpu as T
import test_x3_gpu as X3

pytestmark = pytest.mark.gpu

# case name -> the entry points the case must reach (asserted through the recorder); tests/test_memory_contract_cpu.py checks that
# these sets and tests/test_step_poisoned_gpu.py's together are exactly memcheck.COVERED
REACHES = {
    "dwconv": {"mliis_dwconv_fwd", "mliis_dwconv_bwd_data", "mliis_dwconv_bwd_filter"},
    "dwconv_bn_stage1": {"mliis_dwconv_bwd_data_bn"},
    "conv2d": {"mliis_conv2d_fwd", "mliis_conv2d_bwd_data", "mliis_conv2d_bwd_filter", "mliis_transpose_weights", "mliis_colsum"},
    "stem": {"mliis_stem_conv_fwd", "mliis_stem_conv_fwd_stats", "mliis_stem_conv_bwd_filter"},
    "bn": {"mliis_bn_stats", "mliis_bn_apply", "mliis_bn_bwd", "mliis_bn_stats_partial", "mliis_bn_apply_fused"},
    "bn_pair": {"mliis_bn_apply_fused_pair", "mliis_bn_bwd_pair"},
    "se": {"mliis_se_mlp_fwd", "mliis_se_mlp_bwd"},
    "se_bn": {"mliis_se_bn_bwd_sums", "mliis_se_mlp_bwd_bn"},
    "resize": {"mliis_resize_bilinear_fwd", "mliis_resize_bilinear_bwd"},
    "resize_bwd": {"mliis_resize_bilinear_bwd"},
    "final_conv": {"mliis_final_conv_fwd", "mliis_final_conv_bwd_data", "mliis_final_conv_bwd_filter"},
    "softmax": {"mliis_softmax_ce"},
    "head": {"mliis_head_ce_fused"},
    "rsd_pool": {"mliis_rsd_pool_fwd", "mliis_rsd_pool_bwd"},
    "rsd_concat": {"mliis_rsd_concat_pool"},
    "swish_mask": {"mliis_swish_mask_fwd", "mliis_swish_mask_bwd"},
    "chan": {"mliis_chan_affine"},
    "bnin": {"mliis_conv2d_fwd_bnin"},
    "bwd_data_bn": {"mliis_conv2d_bwd_data_bn"},
    "bwd_data_gate": {"mliis_conv2d_bwd_data_gate"},
    "x3": {"mliis_conv2d_fwd_x3", "mliis_conv2d_bwd_data_x3", "mliis_x3_pack_weights"},
    "dwmarch": {"mliis_dwconv_bn_fwd", "mliis_dwconv_bn_bwd"},
    "dwmarch_bf16": {"mliis_dwconv_bn_fwd"},
    "dwmarch_bwd_bn": {"mliis_mbconv_dw_bwd_march"},
    "mbconv_small": {"mliis_mbconv_dw_fwd_small", "mliis_mbconv_dw_bwd_small"},
    "filter_batched": {"mliis_conv2d_bwd_filter_batched"},
    "fold": {"mliis_fold_batched", "mliis_se_wgrad_batched"},
    "algebra": {"mliis_sgd_fused", "mliis_adam_b1zero_fused", "mliis_axpby", "mliis_lincomb"},
    "shadows": {"mliis_weight_shadows", "mliis_weight_shadows_rng"},
}


def _poisoned(case, fn):
    M.reset_guards()
    with M.poisoned_allocations(), M.record() as reached:
        fn()
    missing = REACHES[case] - reached
    assert not missing, "case {} did not reach {}".format(case, sorted(missing))
    M.assert_guards()


# ------------------------------------------------------------------------------------------------ (a) parity cases under poison
# one or two parameter sets per family, tile-tail shapes where the lists have them (7x9, 15x17, 131x67, N = 37, K = 136, Cout = 20)
PARITY = [
    ("dwconv", lambda: T._dwconv_case(3, 2, 15, 17, 8, 2)),
    ("dwconv", lambda: T._dwconv_case(5, 1, 7, 30, 144, 2)),
    ("dwconv_bn_stage1", lambda: T.test_dwconv_bwd_data_emits_bn_backward_stage1(3, 2, 15, 17, 8)),
    ("conv2d", lambda: T._conv2d_case(1, 1, 7, 9, 96, 24, 3)),
    ("conv2d", lambda: T._conv2d_case(3, 2, 9, 9, 12, 20, 1)),
    ("conv2d", lambda: T._conv2d_case(3, 2, 14, 14, 136, 112, 2)),
    ("stem", lambda: T.test_stem(131, 67, 40)),
    ("bn", lambda: T.test_bn_train_fwd_bwd(1, 0, 40, 3001, 2)),
    ("bn_pair", lambda: T.test_batch_norm_pairs_equal_the_single_launches(300, 136)),
    ("se", lambda: T.test_se(1000, 34, 2, 4)),
    ("se_bn", lambda: T.test_se_and_bn_backward_share_one_pass(40, 10, 3, 196)),
    ("resize", lambda: T.test_resize(7, 5, 20, 13, 8)),
    ("resize_bwd", lambda: T.test_resize_bwd_separable_form_strided_and_accumulating(5, 70, 9, 130, 36, 4)),
    ("final_conv", lambda: T.test_final_conv(136, 77, True)),
    ("softmax", lambda: T.test_softmax_ce(True, 0.1, 9, 7)),
    ("head", lambda: T.test_head_ce_fused_equals_the_four_launch_tail(2, 13, 37, 0.1, 2)),
    ("rsd_pool", lambda: T.test_rsd_pooled_branch_as_border_bias(6, 6, 32, 24, 16, 37)),
    ("rsd_concat", lambda: T.test_rsd_concat_and_pooled_sums(3, 5, 9, 8, 4)),
    ("swish_mask", lambda: T.test_swish_mask_fwd_bwd(True)),
    ("chan", lambda: T.test_chan_affine_broadcast_and_copy()),
    ("bnin", lambda: T.test_conv1x1_with_the_batch_norm_in_front_applied_on_load(8, 56, 56, 24, 144, True, True, "fp32")),
    ("bwd_data_bn", lambda: T.test_conv2d_bwd_data_emits_bn_backward_stage1(5, 28, 240, 40, True, False)),
    ("bwd_data_gate", lambda: T.test_conv2d_bwd_data_emits_gate_gradient_partials(13, 9, 24, 144)),
    ("x3", lambda: X3.test_x3_epilogue_statistics_border_bias_accumulate_and_views(True)),
    ("dwmarch", lambda: DM._case(3, 2, 30, 34, 24, 2, pre=True)),
    ("dwmarch_bwd_bn", lambda: DM.test_depthwise_backward_with_the_batch_norm_backward_formed_on_load(3, 2, 30, 34, 24, 2)),
    ("mbconv_small", lambda: T.test_mbconv_small_fused_fwd_bwd(5, 5, 14, 14, 480, 0)),
    ("mbconv_small", lambda: BF.test_mbconv_small_bf16(3, 40, 2)),
    ("dwmarch_bf16", lambda: BF.test_dwconv_bn_fwd_bf16(3, 2, 28, 48, True)),
    ("filter_batched", lambda: T.test_conv2d_bwd_filter_batched_equals_the_single_calls()),
    ("fold", lambda: T.test_fold_batched_dense_segmented_and_ragged()),
    ("algebra", lambda: T.test_sgd_l2_mask_and_arena_algebra()),
    ("shadows", lambda: T.test_masks_drawn_by_the_weight_shadow_launch_equal_the_mask_launch()),
]


@pytest.mark.parametrize("case,fn", PARITY, ids=["{}-{}".format(c, i) for i, (c, _) in enumerate(PARITY)])
def test_parity_case_on_poisoned_memory(case, fn):
    T.dev()
    _poisoned(case, fn)


# ------------------------------------------------------------------------------------------------ (b) targeted checks
def _x(shape, seed, scale=1.0):
    return T.rnd(*shape, seed=seed, scale=scale)


def test_inputs_are_guarded_and_left_unchanged():
    """Every input sits at the end of a guarded buffer (NaN follows it) and is bitwise unchanged after the call."""
    from mliis_amd import ops
    T.dev()
    M.reset_guards()
    N, H, W, C, k = 2, 15, 17, 24, 3
    x, w = M.guarded_input(_x((N, H, W, C), 1)), M.guarded_input(_x((k, k, C, 1), 2))
    dy = M.guarded_input(_x((N, 8, 9, C), 3))
    ref = ops.dwconv_fwd(x.clone(), w.clone(), 2)
    snap = M.snapshot(x, w, dy)
    with M.poisoned_allocations():
        y = ops.dwconv_fwd(x, w, 2)
        dx = ops.dwconv_bwd_data(dy, w, 2, (H, W))
        dw = ops.dwconv_bwd_filter(x, dy, k, 2)
    snap.assert_unchanged()
    assert torch.equal(y, ref)
    assert not torch.isnan(dx).any() and not torch.isnan(dw).any()
    # dense conv, batch norm, final conv: inputs guarded, outputs finite, inputs bit-identical
    xc, wc, bc = M.guarded_input(_x((3, 7, 9, 136), 4)), M.guarded_input(_x((3, 3, 136, 20), 5, 0.03)), M.guarded_input(_x((20,), 6))
    dyc, dyb = M.guarded_input(_x((3, 7, 9, 20), 7)), M.guarded_input(_x((3, 7, 9, 136), 13))
    g, b = M.guarded_input(_x((136,), 8) * 0.2 + 1), M.guarded_input(_x((136,), 9))
    wf, bf, mask = M.guarded_input(_x((1, 1, 136, 2), 10)), M.guarded_input(_x((2,), 11)), M.guarded_input((_x((3, 7, 9, 136), 12) > 0).float())
    snap = M.snapshot(xc, wc, bc, dyc, dyb, g, b, wf, bf, mask)
    with M.poisoned_allocations():
        outs = [ops.conv2d_fwd(xc, wc, bc, 1), ops.conv2d_bwd_data(dyc, wc, 1), ops.conv2d_bwd_filter(xc, dyc, 3, 1)]
        mean, rstd = ops.bn_stats(xc)
        outs += [mean, rstd, ops.bn_apply(xc, mean, rstd, g, b, post_swish=True)]
        outs += [*ops.bn_bwd(xc, dyb, mean, rstd, g, b)]
        lg = ops.final_conv_fwd(xc, wf, bf, mask)
        outs += [lg, ops.final_conv_bwd_data(lg, wf, 136, mask), *ops.final_conv_bwd_filter(xc, lg, mask)]
    snap.assert_unchanged()
    for o in outs:
        assert not torch.isnan(o).any()
    # squeeze-excite, resize, RSD concat / pooled branch, the fused head
    Ns, Cs, Rs = 3, 40, 10
    s_, w1, b1 = M.guarded_input(_x((Ns, Cs), 20)), M.guarded_input(_x((1, 1, Cs, Rs), 21)), M.guarded_input(_x((Rs,), 22))
    w2, b2 = M.guarded_input(_x((1, 1, Rs, Cs), 23)), M.guarded_input(_x((Cs,), 24))
    dgate = M.guarded_input(_x((Ns, Cs), 25))
    xr, dyr = M.guarded_input(_x((2, 7, 5, 8), 26)), M.guarded_input(_x((2, 20, 13, 8), 27))
    deep, skip = M.guarded_input(_x((3, 5, 5, 8), 28)), M.guarded_input(_x((3, 9, 9, 4), 29))
    wr = M.guarded_input(_x((3, 3, 56, 16), 30, 0.05))
    small = M.guarded_input(_x((2, 13, 13, 2), 31))
    lab = M.guarded_input((_x((2, 37, 37, 1), 32) > 0).double().repeat(1, 1, 1, 2) * torch.tensor([1.0, -1.0], dtype=torch.float64) +
                          torch.tensor([0.0, 1.0], dtype=torch.float64))
    snap = M.snapshot(s_, w1, b1, w2, b2, dgate, xr, dyr, deep, skip, wr, small, lab)
    with M.poisoned_allocations():
        hpre, gate = ops.se_mlp_fwd(s_, w1, b1, w2, b2)
        so = ops.se_mlp_bwd(dgate, gate, s_, hpre, w1, w2, 49)
        outs = [hpre, gate, *so.values(), ops.resize_bilinear_fwd(xr, (20, 13)), ops.resize_bilinear_bwd(dyr, (7, 5))]
        cat = torch.empty(3, 9, 9, 12, device=xr.device)
        pp = torch.empty(ops.rsd_concat_pool_floats(3, 9, 9, 12), device=xr.device)
        ch = ops.rsd_concat_pool(deep, skip, cat, pp)
        pool = torch.empty(3, 12, device=xr.device)
        outs += [cat, ops.rsd_pool_fwd(pp, wr, 44, chunks=ch, scale=1.0 / 81, pool_out=pool), pool]
        ds, lo = torch.empty(2, 13, 13, 2, device=xr.device), torch.empty(4, device=xr.device)
        ops.head_ce_fused(small, lab, torch.arange(2, dtype=torch.int32, device=xr.device), (37, 37), 0.1, ds, lo)
        outs += [ds, lo[:3]]
    snap.assert_unchanged()
    for o in outs:
        assert not torch.isnan(o).any()
    M.assert_guards()


@pytest.mark.parametrize("pad", [4, 8])   # (the kernels take 16-byte aligned rows: other leading dimensions are refused)
def test_channel_slice_views_with_nan_gaps(pad):
    """Every operand a wrapper takes through rows_ld, given as a channel slice of a wider buffer whose gap is NaN: parity with the
    dense call, and the output's gap columns untouched (bitwise)."""
    from mliis_amd import ops
    T.dev()
    M.reset_guards()
    N, H, W, Cin, Cout = 2, 7, 9, 40, 20
    xd, wd = _x((N, H, W, Cin), 1), _x((3, 3, Cin, Cout), 2, 1.0 / math.sqrt(9 * Cin))
    d = T.dev()
    x, w = T.f32(xd, d), T.f32(wd, d)
    xv = M.nan_gap_view(xd, pad, lead=pad)
    # conv family (fwd, bwd data, bwd filter), output into a gap view
    ref = ops.conv2d_fwd(x, w, None, 1)
    out = M.nan_gap_view(torch.zeros(N, H, W, Cout), pad)
    ops.conv2d_fwd(xv, w, None, 1, out=out)
    assert torch.equal(out, ref)
    dy = T.f32(_x((N, H, W, Cout), 3), d)
    dyv = M.nan_gap_view(dy, pad, lead=4)
    refd = ops.conv2d_bwd_data(dy, w, 1)
    outd = M.nan_gap_view(torch.zeros(N, H, W, Cin), pad)
    ops.conv2d_bwd_data(dyv, w, 1, out=outd)
    assert torch.equal(outd, refd)
    T.close(ops.conv2d_bwd_filter(xv, dyv, 3, 1), ops.conv2d_bwd_filter(x, dy, 3, 1), 1e-6, "bwd filter through views")
    # batch norm, chan_affine, chan_split, swish_mask, resize, final conv, colsum
    mean, rstd = ops.bn_stats(x)
    mv, rv = ops.bn_stats(xv)
    assert torch.equal(mean, mv) and torch.equal(rstd, rv)
    g, b = T.f32(_x((Cin,), 4) * 0.2 + 1, d), T.f32(_x((Cin,), 5), d)
    ya = ops.bn_apply(x, mean, rstd, g, b, post_swish=True)
    yv = M.nan_gap_view(torch.zeros(N, H, W, Cin), pad)
    ops.bn_apply(xv, mean, rstd, g, b, post_swish=True, out=yv)
    assert torch.equal(yv, ya)
    part = torch.zeros(ops.bn_stats_partial_floats(N * H * W, Cin), device=d)
    nb = ops.bn_stats_partial(xv, False, part)
    yf = M.nan_gap_view(torch.zeros(N, H, W, Cin), pad)
    m2, r2 = torch.empty_like(mean), torch.empty_like(rstd)
    ops.bn_apply_fused(xv, part, nb, m2, r2, g, b, post_swish=True, out=yf)
    T.close(yf, ya, 1e-5, "bn_apply_fused through views")
    dxb, dgb, dbb = ops.bn_bwd(x, T.f32(_x((N, H, W, Cin), 6), d), mean, rstd, g, b, post_swish=True)
    dxv = M.nan_gap_view(torch.zeros(N, H, W, Cin), pad)
    _, dg2, db2 = ops.bn_bwd(xv, M.nan_gap_view(_x((N, H, W, Cin), 6), pad), mean, rstd, g, b, post_swish=True, dx=dxv)
    T.close(dxv, dxb, 1e-6, "bn_bwd dx through views")
    T.close(dg2, dgb, 1e-6, "bn_bwd dgamma through views")
    S, A = T.f32(_x((N, Cin), 7), d), T.f32(_x((N, Cin), 8), d)
    ca = M.nan_gap_view(torch.zeros(N, H, W, Cin), pad)
    ops.chan_affine(xv, S, A, out=ca)
    assert torch.equal(ca, ops.chan_affine(x, S, A))
    o0, o1 = M.nan_gap_view(torch.zeros(N, H, W, 16), pad), M.nan_gap_view(torch.zeros(N, H, W, Cin - 16), pad)
    ops.chan_split(xv, 16, o0, False, o1, False, A=A)
    r0, r1 = torch.zeros(N, H, W, 16, device=d), torch.zeros(N, H, W, Cin - 16, device=d)
    ops.chan_split(x, 16, r0, False, r1, False, A=A)
    assert torch.equal(o0, r0) and torch.equal(o1, r1)
    mask = T.f32((_x((N, H, W, Cin), 9) > 0).double() * 2, d)
    sm = M.nan_gap_view(torch.zeros(N, H, W, Cin), pad)
    ops.swish_mask_fwd(xv, M.nan_gap_view(mask, pad), out=sm)
    assert torch.equal(sm, ops.swish_mask_fwd(x, mask))
    sb = M.nan_gap_view(torch.zeros(N, H, W, Cin), pad)
    ops.swish_mask_bwd(dxv, xv, M.nan_gap_view(mask, pad), out=sb)
    assert torch.equal(sb, ops.swish_mask_bwd(dxv.contiguous(), x, mask))
    rz = M.nan_gap_view(torch.zeros(N, 13, 11, Cin), pad)
    ops.resize_bilinear_fwd(xv, (13, 11), out=rz)
    assert torch.equal(rz, ops.resize_bilinear_fwd(x, (13, 11)))
    rb = M.nan_gap_view(torch.zeros(N, H, W, Cin), pad)
    ops.resize_bilinear_bwd(M.nan_gap_view(rz, pad), (H, W), out=rb)
    assert torch.equal(rb, ops.resize_bilinear_bwd(rz.contiguous(), (H, W)))
    wf, bf = T.f32(_x((1, 1, Cin, 2), 10), d), T.f32(_x((2,), 11), d)
    lg = ops.final_conv_fwd(xv, wf, bf)
    assert torch.equal(lg, ops.final_conv_fwd(x, wf, bf))
    fd = M.nan_gap_view(torch.zeros(N, H, W, Cin), pad)
    ops.final_conv_bwd_data(lg, wf, Cin, out=fd)
    assert torch.equal(fd, ops.final_conv_bwd_data(lg, wf, Cin))
    dwv, dbv = ops.final_conv_bwd_filter(xv, lg)
    dwr, dbr = ops.final_conv_bwd_filter(x, lg)
    assert torch.equal(dwv, dwr) and torch.equal(dbv, dbr)
    assert torch.equal(ops.colsum(xv, nseg=N), ops.colsum(x, nseg=N))
    # RSD concat: deep / skip as views, cat written through a view
    deep, skip = _x((N, 4, 5, 16), 12), _x((N, H, W, 8), 13)
    catv = M.nan_gap_view(torch.zeros(N, H, W, 24), pad)
    q = ops.rsd_concat_pool_floats(N, H, W, 24)
    pv, pd = torch.zeros(q, device=d), torch.zeros(q, device=d)
    chv = ops.rsd_concat_pool(M.nan_gap_view(deep, pad), M.nan_gap_view(skip, pad, lead=4), catv, pv)
    catd = torch.zeros(N, H, W, 24, device=d)
    chd = ops.rsd_concat_pool(T.f32(deep, d), T.f32(skip, d), catd, pd)
    assert chv == chd and torch.equal(catv, catd) and torch.equal(pv, pd)
    # the 1x1 conv with the batch norm on load: z, a_out and out as views
    Nb, Hb, Cb, Cob = 8, 28, 40, 240
    assert ops.conv2d_fwd_bnin_ok(Nb, Hb, Hb, Cb, Cob)
    zb = _x((Nb, Hb, Hb, Cb), 14)
    wb = T.f32(_x((1, 1, Cb, Cob), 15, 0.1), d)
    gb, bb = T.f32(_x((Cb,), 18) * 0.2 + 1, d), T.f32(_x((Cb,), 19), d)
    part = torch.zeros(ops.bn_stats_partial_floats(Nb * Hb * Hb, Cb), device=d)
    nbk = ops.bn_stats_partial(T.f32(zb, d), False, part)     # (the kernel folds the stage-1 statistics: mean / rstd are outputs)
    ad, od = torch.zeros(Nb, Hb, Hb, Cb, device=d), torch.zeros(Nb, Hb, Hb, Cob, device=d)
    md, rd = torch.zeros(Cb, device=d), torch.zeros(Cb, device=d)
    ops.conv2d_fwd_bnin(T.f32(zb, d), part.clone(), nbk, md, rd, gb, bb, ad, wb, od)
    av, ov = M.nan_gap_view(torch.zeros(Nb, Hb, Hb, Cb), pad), M.nan_gap_view(torch.zeros(Nb, Hb, Hb, Cob), pad)
    mv_, rv_ = torch.zeros(Cb, device=d), torch.zeros(Cb, device=d)
    ops.conv2d_fwd_bnin(M.nan_gap_view(zb, pad, lead=pad), part.clone(), nbk, mv_, rv_, gb, bb, av, wb, ov)
    assert torch.equal(mv_, md) and torch.equal(rv_, rd)
    assert torch.equal(av, ad) and torch.equal(ov, od)
    M.assert_guards()


def _cap_check(what, call, query, used, block):
    """Partial-sum buffers sized by a query.  call(buffer) with exactly `query` floats must take the fused path (returns its block
    count > 0) and keep the guard behind the buffer; with one block (`block` floats) less than the `used` floats that call wrote, the
    library must refuse (MliisError) or take its documented fallback (returns 0 and leaves the buffer untouched) -- never write past
    the capacity."""
    from mliis_amd import ops
    M.reset_guards()
    buf = M.guarded_buffer(query)
    r = call(buf)
    assert r > 0, "{}: the fused path was not taken at exactly the queried size ({} floats)".format(what, query)
    assert r * block <= query, "{}: {} blocks of {} floats reported for a {}-float buffer".format(what, r, block, query)
    M.assert_guards()
    M.reset_guards()
    small = M.guarded_buffer(used - block, fill=0.0)
    try:
        r = call(small)
    except ops.MliisError:
        r = None
    if r is not None:
        assert r == 0, "{}: {} blocks reported for a buffer one block short".format(what, r)
        assert bool((small == 0).all()), what + ": fell back but wrote the buffer"
    M.assert_guards()


def test_capacities_at_the_queried_size_and_one_block_less():
    from mliis_amd import ops
    from mliis_amd._lib import lib
    d = T.dev()
    with M.poisoned_allocations():
        rows, C = 3001 * 2, 40
        x = T.f32(_x((2, 3001, 1, C), 1), d)
        q = ops.bn_stats_partial_floats(rows, C)
        nb = ops.bn_stats_partial(x, False, torch.zeros(q, device=d))
        _cap_check("bn_stats_partial", lambda b: ops.bn_stats_partial(x, False, b), q, nb * 2 * C, 2 * C)
        # depthwise forward with the next batch norm's statistics (the plan sizes it as 16-row groups: plan.py stats_part)
        xd, wd = T.f32(_x((2, 15, 17, 24), 2), d), T.f32(_x((3, 3, 24, 1), 3), d)
        q = max(-(-(2 * 15 * 17) // 16) * 2 * 24, ops.bn_stats_partial_floats(2 * 15 * 17, 24))
        nb = ops.dwconv_fwd(xd, wd, 1, stats_part=torch.zeros(q, device=d))[1]
        _cap_check("dwconv_fwd stats", lambda b: ops.dwconv_fwd(xd, wd, 1, stats_part=b)[1], q, nb * 2 * 24, 2 * 24)
        # large-map depthwise with the batch norm on load: forward statistics and backward slabs, sized by the C block queries
        z = T.f32(_x((2, 30, 34, 24), 4), d)
        fb = lib.raw("mliis_dwconv_bn_fwd_blocks")(2, 30, 34, 24, 3, 2)
        _cap_check("dwconv_bn_fwd stats", lambda b: ops.dwconv_bn_fwd(z, wd, 2, stats_part=b)[1], fb * 2 * 24, fb * 2 * 24, 2 * 24)
        bb = ops.dwconv_bn_bwd_blocks(2, 30, 34, 24, 3, 2)
        dyz = T.f32(_x((2, 15, 17, 24), 5), d)
        _cap_check("dwconv_bn_bwd slabs", lambda b: ops.dwconv_bn_bwd(dyz, z, wd, 2, dw_part=b)[2], bb * 9 * 24, bb * 9 * 24, 9 * 24)
        # stem with statistics
        xs = T.f32(_x((2, 33, 35, 3), 6), d)
        ws_ = T.f32(_x((3, 3, 3, 32), 7), d)
        q = ops.stem_conv_fwd_stats_floats(2, 33, 35, 32)
        nb = ops.stem_conv_fwd(xs, ws_, stats_part=torch.zeros(q, device=d))[1]
        _cap_check("stem_conv_fwd_stats", lambda b: ops.stem_conv_fwd(xs, ws_, stats_part=b)[1], q, nb * 2 * 32, 2 * 32)
        # squeeze-excite + batch-norm backward sums ([N][nblk][5][C]: one block less is one per image)
        z1, da2 = T.f32(_x((3, 14, 14, 40), 8), d), T.f32(_x((3, 14, 14, 40), 9), d)
        mean, rstd = ops.bn_stats(z1)
        g, b_ = torch.ones(40, device=d), torch.zeros(40, device=d)
        q = ops.se_bn_bwd_sums_floats(3, 196, 40)
        nb = ops.se_bn_bwd_sums(z1, da2, mean, rstd, g, b_, torch.zeros(q, device=d))
        _cap_check("se_bn_bwd_sums", lambda bf: ops.se_bn_bwd_sums(z1, da2, mean, rstd, g, b_, bf), q, 3 * nb * 5 * 40, 3 * 5 * 40)
        # RSD concat + pooled sums ([N][chunks][C])
        deep, skip = T.f32(_x((3, 5, 5, 8), 10), d), T.f32(_x((3, 9, 9, 4), 11), d)
        cat = torch.zeros(3, 9, 9, 12, device=d)
        q = ops.rsd_concat_pool_floats(3, 9, 9, 12)
        ch = ops.rsd_concat_pool(deep, skip, cat, torch.zeros(q, device=d))
        _cap_check("rsd_concat_pool", lambda bf: ops.rsd_concat_pool(deep, skip, cat, bf), q, 3 * ch * 12, 3 * 12)


def _ws_check(what, call, query):
    """Workspaces sized by a *_workspace_floats query.  call(ws) returns the outputs; given exactly `query` floats (a guarded buffer
    handed out whole) the outputs are bit-identical to a call on the default workspace and the guard holds; given one float less the
    library refuses (MliisError) or, when the plan does not use the whole workspace, returns the same bits -- never writes past it."""
    from mliis_amd import ops
    ref = [t.clone() for t in call(None)]
    M.reset_guards()
    got = call(M.FixedWorkspace(M.guarded_buffer(query)))
    for a, b in zip(got, ref):
        assert M.bits_equal(a, b), what + ": result differs on a workspace of exactly the queried size"
    M.assert_guards()
    if query == 0:     # (no workspace asked for: the empty buffer above is all the call may touch)
        return
    M.reset_guards()
    try:
        got = call(M.FixedWorkspace(M.guarded_buffer(query - 1)))
    except ops.MliisError:
        got = None
    if got is not None:
        for a, b in zip(got, ref):
            assert M.bits_equal(a, b), what + ": accepted a workspace one float short and returned different results"
    M.assert_guards()


def test_workspace_queries_at_the_queried_size_and_one_less():
    from mliis_amd import ops
    from mliis_amd._lib import lib
    d = T.dev()
    sz = lib.size
    # dense conv, split-K shapes (the workspace holds the K-split partials)
    x, w = T.f32(_x((2, 14, 14, 672), 1), d), T.f32(_x((1, 1, 672, 112), 2, 0.04), d)
    dy = T.f32(_x((2, 14, 14, 112), 3), d)
    _ws_check("conv2d_fwd", lambda ws: [ops.conv2d_fwd(x, w, None, 1, ws=ws)], sz("mliis_conv2d_workspace_floats", 2, 14, 14, 672, 112, 1))
    _ws_check("conv2d_bwd_data", lambda ws: [ops.conv2d_bwd_data(dy, w, 1, ws=ws)], sz("mliis_conv2d_workspace_floats", 2, 14, 14, 112, 672, 1))
    _ws_check("conv2d_bwd_filter", lambda ws: [ops.conv2d_bwd_filter(x, dy, 1, 1, ws=ws)],
              sz("mliis_conv2d_bwd_filter_workspace_floats", 2, 14, 14, 672, 112, 1))
    # split-product convs
    x3, w3 = T.f32(_x((2, 14, 14, 224), 4), d), T.f32(_x((3, 3, 224, 112), 5, 0.02), d)
    dy3 = T.f32(_x((2, 14, 14, 112), 6), d)
    imf, imb = ops.x3_image_of(w3, "fwd"), ops.x3_image_of(w3, "bwd")
    _ws_check("conv2d_fwd_x3", lambda ws: [ops.conv2d_fwd_x3(x3, imf, 3, 112, ws=ws)], sz("mliis_conv2d_x3_workspace_floats", 2, 14, 14, 224, 112, 3))
    _ws_check("conv2d_bwd_data_x3", lambda ws: [ops.conv2d_bwd_data_x3(dy3, imb, 3, 224, ws=ws)],
              sz("mliis_conv2d_x3_workspace_floats", 2, 14, 14, 112, 224, 3))
    # stem and depthwise filter gradients
    xs, dzs = T.f32(_x((2, 33, 35, 3), 7), d), T.f32(_x((2, 17, 18, 32), 8), d)
    _ws_check("stem_conv_bwd_filter", lambda ws: [ops.stem_conv_bwd_filter(xs, dzs, ws=ws)],
              sz("mliis_stem_conv_bwd_filter_workspace_floats", 2, 33, 35, 32))
    xd, dyd = T.f32(_x((2, 15, 17, 24), 9), d), T.f32(_x((2, 8, 9, 24), 10), d)
    _ws_check("dwconv_bwd_filter", lambda ws: [ops.dwconv_bwd_filter(xd, dyd, 3, 2, ws=ws)],
              sz("mliis_dwconv_bwd_filter_workspace_floats", 2, 15, 17, 24, 3, 2))
    # column reductions (colreduce): batch norm statistics and backward, colsum, the final conv's filter gradient
    xb = T.f32(_x((2, 3001, 1, 40), 11), d)
    dyb = T.f32(_x((2, 3001, 1, 40), 12), d)
    g, b = T.f32(_x((40,), 13) * 0.2 + 1, d), T.f32(_x((40,), 14), d)
    cr = sz("mliis_colreduce_workspace_floats", 6002, 40, 1, 2)
    _ws_check("bn_stats", lambda ws: list(ops.bn_stats(xb, ws=ws)), cr)
    m, r = ops.bn_stats(xb)
    _ws_check("bn_bwd", lambda ws: list(ops.bn_bwd(xb, dyb, m, r, g, b, ws=ws)), cr)
    _ws_check("colsum", lambda ws: [ops.colsum(xb, nseg=2, ws=ws)], sz("mliis_colreduce_workspace_floats", 3001, 40, 2, 1))
    wf = T.f32(_x((1, 1, 40, 2), 15), d)
    lg = ops.final_conv_fwd(xb, wf, T.f32(_x((2,), 16), d))
    _ws_check("final_conv_bwd_filter", lambda ws: list(ops.final_conv_bwd_filter(xb, lg, ws=ws)), cr)
    # bn_bwd's per-chunk column sums of dx (dxsum_part, bn_bwd_dxsum_floats)
    q = ops.bn_bwd_dxsum_floats(6002, 40)

    def dxsum(buf):
        ops.bn_bwd(xb, dyb, m, r, g, b, dxsum_part=buf)
        return [buf.clone()]
    ref = dxsum(torch.zeros(q, device=d))
    M.reset_guards()
    assert M.bits_equal(dxsum(M.guarded_buffer(q))[0], ref[0])
    M.assert_guards()
    M.reset_guards()
    with pytest.raises(ops.MliisError):
        dxsum(M.guarded_buffer(q - 1))
    M.assert_guards()
    # loss: softmax cross-entropy, the fused head, the RSD pooled branch's backward
    S, Hh = 3, 24
    logits = T.f32(_x((S, Hh, Hh, 2), 17), d)
    lab = T.f32((_x((S, Hh, Hh, 1), 18) > 0).double().repeat(1, 1, 1, 2) * torch.tensor([1.0, -1.0], dtype=torch.float64) +
                torch.tensor([0.0, 1.0], dtype=torch.float64), d)
    idx = torch.arange(S, dtype=torch.int32, device=d)
    def sce(ws):
        out, dl, _ = ops.softmax_ce(logits, lab, idx, 0.1, True, ws=ws)
        return [out[:1], dl]
    _ws_check("softmax_ce", sce, sz("mliis_softmax_ce_workspace_floats", S, Hh, Hh))
    small = T.f32(_x((S, 6, 6, 2), 19), d)

    def head(ws):
        ds, lo = torch.zeros(S, 6, 6, 2, device=d), torch.zeros(4, device=d)
        ops.head_ce_fused(small, lab, idx, (Hh, Hh), 0.1, ds, lo, ws=ws)
        return [ds, lo[:3]]
    _ws_check("head_ce_fused", head, sz("mliis_head_ce_fused_workspace_floats", S, 6, 6))
    pool, wr = T.f32(_x((2, 24), 20), d), T.f32(_x((3, 3, 56, 16), 21, 0.05), d)
    dz = T.f32(_x((2, 6, 6, 16), 22), d)

    def rsd_bwd(ws):
        tot, dwr, dbr = torch.zeros(2, 16, device=d), torch.zeros(3, 3, 56, 16, device=d), torch.zeros(16, device=d)
        dp = ops.rsd_pool_bwd(dz, tot, pool, wr, 32, dwr, dbr, ws=ws)
        return [dp, tot, dwr, dbr]
    _ws_check("rsd_pool_bwd", rsd_bwd, sz("mliis_rsd_pool_bwd_workspace_floats", 2, 16))


def test_dirty_workspace_second_call_is_bit_identical():
    """The second call gets the first call's leftover workspace and partial buffers (not NaN): bit-identical results."""
    from mliis_amd import ops
    d = T.dev()
    M.reset_guards()
    with M.poisoned_allocations():
        ws = ops.Workspace(d, 1 << 16)
        x, w = T.f32(_x((8, 14, 14, 136), 1), d), T.f32(_x((3, 3, 136, 112), 2, 0.03), d)
        dy = T.f32(_x((8, 14, 14, 112), 3), d)
        xd, wd = T.f32(_x((2, 15, 17, 24), 4), d), T.f32(_x((3, 3, 24, 1), 5), d)
        dyd = T.f32(_x((2, 8, 9, 24), 6), d)
        part = torch.empty(1 << 16, device=d)

        def run():
            o = [ops.conv2d_fwd(x, w, None, 2, ws=ws), ops.conv2d_bwd_data(dy, w, 2, ws=ws), ops.conv2d_bwd_filter(x, dy, 3, 2, ws=ws)]
            o += list(ops.bn_stats(x, ws=ws)) + [ops.colsum(dy, nseg=8, ws=ws)]
            y, nb = ops.dwconv_fwd(xd, wd, 2, stats_part=part)
            o += [y, part[:nb * 2 * 24].clone(), ops.dwconv_bwd_filter(xd, dyd, 3, 2, ws=ws)]
            o += [ops.dwconv_bn_bwd(dyd, xd, wd, 2, ws=ws)[1]]
            return [t.clone() for t in o]

        first = run()
        second = run()
    for i, (a, b) in enumerate(zip(first, second)):
        assert M.bits_equal(a, b), "output {} differs on a dirty workspace".format(i)
        assert not torch.isnan(a).any(), "output {} read poisoned memory".format(i)
    M.assert_guards()
