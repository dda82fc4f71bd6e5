"""Layout contract of the wrappers in mliis_amd/ops.py.  Every tensor argument is either honoured as a view (the wrapper passes a row
stride: parity with the dense call) or refused with MliisError before anything is launched; a caller's out= of the wrong shape or dtype
is refused.  The wrong out= is a slightly smaller tensor followed by a guard of at least one full output (tests/memcheck.py): a call
that is not refused writes into that guard and fails the guard check, never past the allocation."""
import pytest
import torch

import memcheck as M
import test_ops_gpu as T
from mliis_amd._lib import MliisError

pytestmark = pytest.mark.gpu


def _r(shape, seed, scale=1.0):
    return T.f32(T.rnd(*shape, seed=seed, scale=scale), T.dev())


def _slice(t, pad=4):
    """channel-slice view of t (a [..., C + pad] buffer, NaN in the gap)"""
    return M.nan_gap_view(t, pad)


def _strided(t):
    """the same values, not dense: every other element of a buffer twice the size (the gaps hold the guard NaN)"""
    buf = M.fill_guard(torch.zeros(2 * t.numel(), dtype=t.dtype, device=t.device))
    strides = [1] * t.dim()
    for i in range(t.dim() - 2, -1, -1):
        strides[i] = strides[i + 1] * t.shape[i + 1]
    v = torch.as_strided(buf, tuple(t.shape), tuple(2 * s for s in strides))
    v.copy_(t)
    return v


def _refuses(fn):
    with pytest.raises(MliisError):
        fn()


def test_depthwise_and_stem_refuse_views_they_would_read_as_dense():
    from mliis_amd import ops
    M.reset_guards()
    x, w = _r((2, 15, 17, 24), 1), _r((3, 3, 24, 1), 2)
    dy = _r((2, 8, 9, 24), 3)
    _refuses(lambda: ops.dwconv_fwd(_slice(x), w, 2))
    _refuses(lambda: ops.dwconv_fwd(x, _strided(w), 2))
    _refuses(lambda: ops.dwconv_bwd_data(_slice(dy), w, 2, (15, 17)))
    _refuses(lambda: ops.dwconv_bwd_data(dy, _strided(w), 2, (15, 17)))
    _refuses(lambda: ops.dwconv_bwd_filter(_slice(x), dy, 3, 2))
    _refuses(lambda: ops.dwconv_bwd_filter(x, _slice(dy), 3, 2))
    _refuses(lambda: ops.dwconv_bn_fwd(_slice(x), w, 2))
    _refuses(lambda: ops.dwconv_bn_bwd(_slice(dy), x, w, 2))
    xs, ws_ = _r((2, 17, 19, 3), 4), _r((3, 3, 3, 32), 5)
    _refuses(lambda: ops.stem_conv_fwd(_slice(xs, 1), ws_))
    _refuses(lambda: ops.stem_conv_fwd(xs, _strided(ws_)))
    _refuses(lambda: ops.stem_conv_bwd_filter(xs, _slice(_r((2, 9, 10, 32), 6))))
    M.assert_guards()


def test_dense_operands_of_the_other_wrappers_are_refused_as_views():
    from mliis_amd import ops
    M.reset_guards()
    N, C, R = 3, 40, 10
    x = _r((N, 7, 9, C), 1)
    wf, bf = _r((1, 1, C, 2), 2), _r((2,), 3)
    mask = (_r((N, 7, 9, C), 4) > 0).float()
    _refuses(lambda: ops.final_conv_fwd(x, wf, bf, _slice(mask)))
    _refuses(lambda: ops.final_conv_fwd(x, _strided(wf), bf))
    lg = ops.final_conv_fwd(x, wf, bf, mask)
    _refuses(lambda: ops.final_conv_bwd_data(_slice(lg, 2), wf, C, mask))
    _refuses(lambda: ops.final_conv_bwd_data(lg, wf, C, _slice(mask)))
    _refuses(lambda: ops.final_conv_bwd_filter(x, _slice(lg, 2), mask))
    s = _r((N, C), 5)
    w1, b1, w2, b2 = _r((1, 1, C, R), 6), _r((R,), 7), _r((1, 1, R, C), 8), _r((C,), 9)
    _refuses(lambda: ops.se_mlp_fwd(_slice(s), w1, b1, w2, b2))
    _refuses(lambda: ops.se_mlp_fwd(s, _strided(w1), b1, w2, b2))
    _refuses(lambda: ops.se_mlp_fwd(s, w1, b1, _strided(w2), b2))
    # dense-conv weights: the backward-data kernel reads w as HWIO without a stride, the forward its K-contiguous copy
    xc, wc = _r((2, 7, 9, 24), 10), _r((3, 3, 24, 20), 11, 0.05)
    _refuses(lambda: ops.conv2d_bwd_data(_r((2, 7, 9, 20), 12), _strided(wc)))
    _refuses(lambda: ops.conv2d_fwd(xc, wc, None, 1, wt=_strided(ops.hwoi(wc))))
    # conv2d_fwd builds its K-contiguous copy from any layout of w: a strided w gives the dense result
    assert torch.equal(ops.conv2d_fwd(xc, _strided(wc)), ops.conv2d_fwd(xc, wc))
    lo = _r((2, 9, 7, 2), 13)
    _refuses(lambda: ops.softmax_ce(_slice(lo, 2), torch.zeros(2, 9, 7, 2, device=lo.device)))
    th, g = _r((64,), 14), _r((64,), 15)
    _refuses(lambda: ops.sgd_fused(th, _r((128,), 16)[::2], 0.1))
    _refuses(lambda: ops.axpby(0.5, _r((128,), 17)[::2], 1.0, th))
    _refuses(lambda: ops.lincomb(0.5, th, 1.0, g, _r((128,), 18)[::2]))
    M.assert_guards()


def test_strided_operands_are_honoured():
    """The operands the wrappers pass with a row stride: channel slices give the dense result (details, NaN gaps and all output
    families: tests/test_memory_contract_gpu.py::test_channel_slice_views_with_nan_gaps)."""
    from mliis_amd import ops
    M.reset_guards()
    x, w = _r((2, 7, 9, 24), 1), _r((1, 1, 24, 20), 2, 0.1)
    assert torch.equal(ops.conv2d_fwd(_slice(x), w), ops.conv2d_fwd(x, w))
    assert torch.equal(ops.resize_bilinear_fwd(_slice(x), (5, 4)), ops.resize_bilinear_fwd(x, (5, 4)))
    assert torch.equal(ops.colsum(_slice(x), nseg=2), ops.colsum(x, nseg=2))
    wf, bf = _r((1, 1, 24, 2), 3), _r((2,), 4)
    assert torch.equal(ops.final_conv_fwd(_slice(x), wf, bf), ops.final_conv_fwd(x, wf, bf))
    m, r = ops.bn_stats(x)
    assert all(torch.equal(a, b) for a, b in zip(ops.bn_stats(_slice(x)), (m, r)))
    M.assert_guards()


def test_wrong_caller_out_is_refused():
    from mliis_amd import ops
    M.reset_guards()
    N, H, W, C = 2, 7, 9, 24
    x, w = _r((N, H, W, C), 1), _r((3, 3, C, 1), 2)
    short = M.guarded_out_short
    _refuses(lambda: ops.dwconv_fwd(x, w, 1, out=short((N, H, W, C))))
    _refuses(lambda: ops.dwconv_fwd(x, w, 1, out=M.guarded_wrong_dtype((N, H, W, C), torch.float16)))
    _refuses(lambda: ops.dwconv_bwd_data(x, w, 1, (H, W), out=short((N, H, W, C))))
    _refuses(lambda: ops.dwconv_bwd_filter(x, x, 3, 1, out=short((3, 3, C)).unsqueeze(-1)))
    _refuses(lambda: ops.resize_bilinear_fwd(x, (13, 11), out=short((N, 13, 11, C))))
    _refuses(lambda: ops.resize_bilinear_fwd(x, (13, 11), out=M.guarded_wrong_dtype((N, 13, 11, C), torch.float16)))
    _refuses(lambda: ops.resize_bilinear_bwd(x, (5, 4), out=short((N, 5, 4, C))))
    wf, bf = _r((1, 1, C, 2), 3), _r((2,), 4)
    _refuses(lambda: ops.final_conv_fwd(x, wf, bf, out=short((N, H, W, 2))))
    _refuses(lambda: ops.final_conv_fwd(x, wf, bf, out=M.guarded_wrong_dtype((N, H, W, 2), torch.float16)))
    lg = ops.final_conv_fwd(x, wf, bf)
    _refuses(lambda: ops.final_conv_bwd_data(lg, wf, C, out=short((N, H, W, C))))
    wc = _r((1, 1, C, 20), 5, 0.1)
    _refuses(lambda: ops.conv2d_fwd(x, wc, out=short((N, H, W, 20))))
    _refuses(lambda: ops.conv2d_bwd_data(_r((N, H, W, 20), 6), wc, out=short((N, H, W, C))))
    _refuses(lambda: ops.conv2d_bwd_filter(x, _r((N, H, W, 20), 6), 1, out=short((1, 1, C, 20))))
    m, r = ops.bn_stats(x)
    g, b = _r((C,), 7), _r((C,), 8)
    _refuses(lambda: ops.bn_apply(x, m, r, g, b, out=short((N, H, W, C))))
    _refuses(lambda: ops.bn_stats(x, mean=short((C,))))
    _refuses(lambda: ops.bn_bwd(x, x, m, r, g, b, dx=short((N, H, W, C))))
    _refuses(lambda: ops.colsum(x, nseg=N, out=short((N, C))))
    _refuses(lambda: ops.chan_affine(x, out=short((N, H, W, C))))
    _refuses(lambda: ops.swish_mask_fwd(x, out=short((N, H, W, C))))
    s = _r((N, C), 9)
    w1, b1, w2, b2 = _r((1, 1, C, 6), 10), _r((6,), 11), _r((1, 1, 6, C), 12), _r((C,), 13)
    _refuses(lambda: ops.se_mlp_fwd(s, w1, b1, w2, b2, gate=short((N, C))))
    lo = _r((N, H, W, 2), 14)
    _refuses(lambda: ops.softmax_ce(lo, torch.zeros_like(lo), dlogits=short((N, H, W, 2))))
    M.assert_guards()


def _u8_strided(n):
    """a byte buffer of n elements that is not dense (every other byte)"""
    return torch.zeros(2 * n, dtype=torch.uint8, device="cuda")[::2]


def test_fused_and_batched_wrappers_refuse_what_their_kernels_cannot_take():
    """The wrappers of the fused MBConv, SE, RSD, head, optimizer and descriptor-table launches: an operand the kernel reads as dense,
    given strided or as a channel slice, and a caller's output of the wrong shape are refused before anything is launched."""
    from mliis_amd import ops
    M.reset_guards()
    short = M.guarded_out_short
    N, H, W, C, R = 2, 6, 6, 8, 4
    z, z1, a1, da2 = _r((N, H, W, C), 1), _r((N, H, W, C), 2), _r((N, H, W, C), 3), _r((N, H, W, C), 4)
    w = _r((3, 3, C, 1), 5)
    v = [_r((C,), 10 + i) for i in range(8)]
    s, gate, chan_add = _r((N, C), 20), _r((N, C), 21), _r((N, C), 22)
    bn6 = (v[0], v[1], v[2], v[3], None, None)
    bn4 = (v[0], v[1], v[2], v[3])
    dw = _r((3, 3, C, 1), 6)
    # small-map fused depthwise halves
    _refuses(lambda: ops.mbconv_dw_fwd_small(z, None, 0, bn6, _strided(w), bn6, z1, a1, s))
    _refuses(lambda: ops.mbconv_dw_fwd_small(_slice(z), None, 0, bn6, w, bn6, z1, a1, s))
    _refuses(lambda: ops.mbconv_dw_fwd_small(z, None, 0, (v[0], _strided(v[1]), v[2], v[3], None, None), w, bn6, z1, a1, s))
    _refuses(lambda: ops.mbconv_dw_bwd_small(da2, gate, chan_add, z1, bn4, _strided(w), z, bn4, v[4], v[5], dw, v[6], v[7], a1))
    _refuses(lambda: ops.mbconv_dw_bwd_small(_slice(da2), gate, chan_add, z1, bn4, w, z, bn4, v[4], v[5], dw, v[6], v[7], a1))
    _refuses(lambda: ops.mbconv_dw_bwd_small(da2, gate, chan_add, z1, bn4, w, z, bn4, v[4], v[5], _strided(dw), v[6], v[7], a1))
    # large-map depthwise backward
    part = _r((4096,), 23)
    stage1 = _r((N, 2, C), 24)
    _refuses(lambda: ops.mbconv_dw_bwd_march(da2, z1, bn4, gate, chan_add, stage1, v[4], v[5], z, bn4, _strided(w), 1, a1, part, part))
    _refuses(lambda: ops.mbconv_dw_bwd_march(da2, z1, bn4, gate, chan_add, stage1, v[4], v[5], z, bn4, w, 1, short((N, H, W, C)), part, part))
    _refuses(lambda: ops.dwconv_bn_bwd(da2, z, w, 1, dw=short((3, 3, C)).unsqueeze(-1)))
    _refuses(lambda: ops.dwconv_bn_bwd(da2, z, w, 1, dw_part=_r((8192,), 25)[::2]))
    # 1x1 conv with the batch norm on load: weights (K-contiguous copy), a_out and out
    w1x1 = _r((1, 1, C, 16), 26, 0.2)
    wt = ops.hwoi(w1x1)
    zp = _r((4096,), 27)
    _refuses(lambda: ops.conv2d_fwd_bnin(z, zp, 0, v[2], v[3], v[0], v[1], a1, w1x1, _r((N, H, W, 16), 28), wt=_strided(wt)))
    _refuses(lambda: ops.conv2d_fwd_bnin(z, zp, 0, v[2], v[3], v[0], v[1], short((N, H, W, C)), w1x1, _r((N, H, W, 16), 28), wt=wt))
    _refuses(lambda: ops.conv2d_fwd_bnin(z, zp, 0, v[2], v[3], v[0], v[1], a1, w1x1, short((N, H, W, 16)), wt=wt))
    _refuses(lambda: ops.conv2d_fwd_bnin(z, zp, 0, v[2], _strided(v[3]), v[0], v[1], a1, w1x1, _r((N, H, W, 16), 28), wt=wt))
    # split-product convs: the weight image and the output
    xc = _r((N, H, W, 64), 29)
    wc = _r((3, 3, 64, 64), 30, 0.05)
    img = ops.x3_image_of(wc, "fwd")
    _refuses(lambda: ops.conv2d_fwd_x3(xc, _u8_strided(img.numel()), 3, 64))
    _refuses(lambda: ops.conv2d_fwd_x3(xc, img, 3, 64, out=short((N, H, W, 64))))
    imb = ops.x3_image_of(wc, "bwd")
    _refuses(lambda: ops.conv2d_bwd_data_x3(_r((N, H, W, 64), 31), _u8_strided(imb.numel()), 3, 64))
    _refuses(lambda: ops.conv2d_bwd_data_x3(_r((N, H, W, 64), 31), imb, 3, 64, out=short((N, H, W, 64))))
    # batch norm: fused apply, the pairs
    pb = _r((4096,), 32)
    _refuses(lambda: ops.bn_apply_fused(z, pb, 0, v[2], v[3], v[0], v[1], out=short((N, H, W, C))))
    _refuses(lambda: ops.bn_apply_fused(z, pb, 0, v[2], v[3], _strided(v[0]), v[1]))
    pair = lambda m: [(z, pb, 0, m, v[3], v[0], v[1], None, a1), (z1, pb, 0, v[2], v[3], v[0], v[1], None, da2)]  # noqa: E731
    _refuses(lambda: ops.bn_apply_fused_pair(pair(_strided(v[2]))))
    bpair = lambda g: [(z, da2, v[2], v[3], g, v[1], a1, v[4], v[5], None), (z1, da2, v[2], v[3], v[0], v[1], _r((N, H, W, C), 33), v[6], v[7], None)]  # noqa: E731
    _refuses(lambda: ops.bn_bwd_pair(bpair(_strided(v[0]))))
    # squeeze-excite
    w1, w2, hpre = _r((1, 1, C, R), 34), _r((1, 1, R, C), 35), _r((N, R), 36)
    _refuses(lambda: ops.se_mlp_bwd(gate, gate, s, hpre, _strided(w1), w2, H * W))
    _refuses(lambda: ops.se_mlp_bwd(gate, gate, _slice(s), hpre, w1, w2, H * W))
    _refuses(lambda: ops.se_bn_bwd_sums(z1, da2, v[2], v[3], v[0], v[1], _r((8192,), 37)[::2]))
    _refuses(lambda: ops.se_bn_bwd_sums(z1, da2, v[2], _strided(v[3]), v[0], v[1], _r((4096,), 37)))
    outs = dict(dpre1=_r((N, R), 38), dpre2=_r((N, C), 39), chan_add=_r((N, C), 40))
    _refuses(lambda: ops.se_mlp_bwd_bn(_r((4096,), 41), 1, gate, hpre, w1, _strided(w2), H * W, outs, stage1))
    _refuses(lambda: ops.se_mlp_bwd_bn(_r((4096,), 41), 1, gate, hpre, w1, w2, H * W, dict(outs, chan_add=_slice(chan_add)), stage1))
    # RSD pooled branch and concat
    pool, wr = _r((N, 24), 42), _r((3, 3, 56, 16), 43, 0.05)
    _refuses(lambda: ops.rsd_pool_fwd(pool, wr, 32, out=short((N, 9, 16))))
    _refuses(lambda: ops.rsd_pool_fwd(pool, _strided(wr), 32))
    _refuses(lambda: ops.rsd_pool_fwd(_slice(pool), wr, 32))
    dz, tot = _r((N, H, W, 16), 44), _r((N, 16), 45)
    dwr = _r((3, 3, 56, 16), 46)
    _refuses(lambda: ops.rsd_pool_bwd(dz, tot, pool, wr, 32, dwr, dpool=short((N, 24))))
    _refuses(lambda: ops.rsd_pool_bwd(dz, tot, pool, _strided(wr), 32, dwr))
    deep, skip = _r((N, 3, 3, 8), 47), _r((N, H, W, 4), 48)
    cat = _r((N, H, W, 12), 49)
    _refuses(lambda: ops.rsd_concat_pool(deep, skip, cat, _r((8192,), 50)[::2]))
    _refuses(lambda: ops.rsd_concat_pool(deep, skip, short((N, H, W, 12)), _r((4096,), 50)))
    # head, DARC1, optimizers
    small = _r((N, 5, 5, 2), 51)
    labels = _r((N, 20, 20, 2), 52)
    idx = torch.arange(N, dtype=torch.int32, device=small.device)
    lo4 = _r((4,), 53)
    _refuses(lambda: ops.head_ce_fused(_slice(small, 2), labels, idx, (20, 20), 0.0, _r((N, 5, 5, 2), 54), lo4))
    _refuses(lambda: ops.head_ce_fused(small, labels, idx, (20, 20), 0.0, short((N, 5, 5, 2)), lo4))
    lg = _r((N, 9, 7, 2), 55)
    _refuses(lambda: ops.darc1(_slice(lg, 2), 1e-3, dlogits=_r((N, 9, 7, 2), 56), out=lo4))
    _refuses(lambda: ops.darc1(lg, 1e-3, dlogits=short((N, 9, 7, 2)), out=lo4))
    th, g, vv = _r((64,), 57), _r((64,), 58), _r((64,), 59)
    st = torch.zeros(1, device=th.device)
    _refuses(lambda: ops.adam_b1zero_fused(th, g, _r((128,), 60)[::2], st, 1e-3))
    _refuses(lambda: ops.adam_b1zero_fused(th, short((64,)), vv, st, 1e-3))
    # chan_split / swish_mask_bwd outputs, stem filter-gradient output
    _refuses(lambda: ops.chan_split(z, 3, short((N, H, W, 3)), False, _r((N, H, W, 5), 61), False))
    _refuses(lambda: ops.chan_split(z, 3, _r((N, H, W, 3), 62), False, short((N, H, W, 5)), False))
    _refuses(lambda: ops.swish_mask_bwd(da2, z, out=short((N, H, W, C))))
    xs = _r((N, 9, 9, 3), 63)
    _refuses(lambda: ops.stem_conv_bwd_filter(xs, _r((N, 5, 5, 16), 64), out=short((3, 3, 3, 16))))
    # descriptor-table launches: the tables and the buffers they index are dense
    desc = torch.tensor([[0, 9, C, 16]], dtype=torch.int32, device=th.device)
    src, dst = _r((9 * C * 16,), 65), _r((9 * C * 16,), 66)
    _refuses(lambda: ops.transpose_weights(src, _r((2 * 9 * C * 16,), 67)[::2], desc))
    _refuses(lambda: ops.transpose_weights(src, dst, torch.zeros(1, 8, dtype=torch.int32, device=th.device)[:, ::2]))
    _refuses(lambda: ops.fold_batched(src, dst, torch.zeros(1, 16, dtype=torch.int64, device=th.device)[:, ::2], 1))
    _refuses(lambda: ops.se_wgrad_batched(torch.zeros(1, 24, dtype=torch.int64, device=th.device)[:, ::2], 1))
    _refuses(lambda: ops.copy_words(torch.arange(8, dtype=torch.int32), torch.zeros(16, dtype=torch.int32, device=th.device)[::2]))
    _refuses(lambda: ops.copy_words(torch.arange(8, dtype=torch.int32), torch.zeros(4, dtype=torch.int32, device=th.device)))
    fb = ops.FilterBatch(th.device)
    _refuses(lambda: fb.add(xc, _r((N, H, W, 32), 68), 3, 1, _r((2 * 9 * 64 * 32 * 8,), 69)[::2]))
    M.assert_guards()
