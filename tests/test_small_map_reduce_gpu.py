"""The filter-gradient reduction of mliis_mbconv_dw_bwd_small (two DPP levels per quad, the 16 quad sums of every wave through LDS, rows
and waves folded in a fixed order) at the places such a fold can go wrong: part of one wave with partial quads, ragged rows, a last wave
that is partly idle, 448 of 512 lanes, all 512 lanes at the largest eligible map -- for every (k, V) instance, against the float64
oracle + autograd under the 2e-4 bound of test_ops_gpu.test_mbconv_small_fused_fwd_bwd, and bit for bit against itself: a second call,
the group-blocked operands, and other output buffers."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import efficientlab_ref as R  # noqa: E402
from test_ops_gpu import close, dev, f32, nchw, nhwc, rnd  # noqa: E402

SHAPES = [(2, 2, 3, 16),     # 6 strips: part of one wave, partial quads
          (3, 7, 9, 8),      # ragged rows, 54 strips
          (5, 14, 14, 8),    # 280 strips: a last wave with 24 live lanes
          (8, 14, 14, 8),    # 448 of 512 lanes
          (8, 16, 16, 8)]    # all 512 lanes, the largest eligible map


@functools.lru_cache(maxsize=None)
def _oracle(k, N, H, W, C):
    """Inputs (float64, seeded) and the float64 gradients of one layer; computed once per (k, shape), shared by the V cases, never written."""
    from mliis_amd.spec import BN_EPS
    z0 = (rnd(N, H, W, C, seed=1) * 1.5 + 0.3).requires_grad_(True)
    wd = rnd(k, k, C, 1, seed=2, scale=0.4).requires_grad_(True)
    g0, b0 = (1 + 0.2 * rnd(C, seed=3)).requires_grad_(True), (0.3 * rnd(C, seed=4)).requires_grad_(True)
    g1, b1 = (1 + 0.2 * rnd(C, seed=5)).requires_grad_(True), (0.3 * rnd(C, seed=6)).requires_grad_(True)
    gate, cadd, da2 = torch.sigmoid(rnd(N, C, seed=7)), 0.01 * rnd(N, C, seed=8), rnd(N, H, W, C, seed=9)

    def bn_ref(x, g, b):
        m = x.mean(dim=(0, 1, 2))
        v = ((x - m) ** 2).mean(dim=(0, 1, 2))
        return (x - m) / torch.sqrt(v + BN_EPS) * g + b
    a0 = R.swish(bn_ref(z0, g0, b0))
    z1 = nhwc(R.conv2d_same(nchw(a0), wd, 1, groups=C))
    a1 = R.swish(bn_ref(z1, g1, b1))
    up = da2 * gate[:, None, None, :] + cadd[:, None, None, :]
    grads = torch.autograd.grad((a1 * up).sum(), [z0, wd, g0, b0, g1, b1])
    ins = tuple(t.detach() for t in (z0, wd, g0, b0, g1, b1, gate, cadd, da2))
    return ins, dict(zip(("dz0", "dw", "dg0", "db0", "dg1", "db1"), (g.detach() for g in grads)))


@pytest.mark.parametrize("N,H,W,C", SHAPES)
@pytest.mark.parametrize("k,V", [(3, 2), (3, 4), (5, 2), (5, 4)])
def test_small_map_filter_gradient_fold(k, V, N, H, W, C):
    from mliis_amd import ops
    d = dev()
    assert ops.mbconv_dw_small_supported(N, H, W, C, k, 1)
    (z0, wd, g0, b0, g1, b1, gate, cadd, da2), ref = _oracle(k, N, H, W, C)
    z0d, wdd, da2d, gated, caddd = f32(z0, d), f32(wd, d), f32(da2, d), f32(gate, d), f32(cadd, d)
    bn0, bn1 = (f32(g0, d), f32(b0, d)), (f32(g1, d), f32(b1, d))
    part = torch.zeros(1 << 14, device=d)
    nblk = ops.bn_stats_partial(z0d, False, part)
    st = [torch.zeros(C, device=d) for _ in range(4)]

    def forward(z0in, blocked):
        z1, a1, s = torch.zeros(N, H, W, C, device=d), torch.zeros(N, H, W, C, device=d), torch.zeros(N, C, device=d)
        kw = dict(z0_blocked=z0in if blocked == "in" else torch.zeros_like(z0d), z1_blocked=True) if blocked else {}
        ops.mbconv_dw_fwd_small(z0in, part, nblk, bn0 + (st[0], st[1], None, None), wdd, bn1 + (st[2], st[3], None, None), z1, a1, s,
                                group_width=V, **kw)
        return z1, kw.get("z0_blocked")

    def backward(da2in, z1, fill, **kw):
        o = dict(dg1=torch.full((C,), fill, device=d), db1=torch.full((C,), fill, device=d), dw=torch.full((k, k, C, 1), fill, device=d),
                 dg0=torch.full((C,), fill, device=d), db0=torch.full((C,), fill, device=d), dz0=torch.full((N, H, W, C), fill, device=d))
        ops.mbconv_dw_bwd_small(da2in, gated, caddd, z1, (st[2], st[3]) + bn1, wdd, z0d, (st[0], st[1]) + bn0, o["dg1"], o["db1"], o["dw"],
                                o["dg0"], o["db0"], o["dz0"], group_width=V, **kw)
        return o

    z1d, _ = forward(z0d, None)
    outs = backward(da2d, z1d, 9.0)
    for name in ("dw", "dz0", "dg0", "db0", "dg1", "db1"):
        close(outs[name], ref[name], 2e-4, "small bwd " + name)
    # a second call, into other buffers with another fill: the same bits (fixed addition order; nothing read from an output)
    again = backward(da2d, z1d, -3.0)
    for name in outs:
        assert torch.equal(again[name], outs[name]), "second call: " + name
    # dw when the operands and every other output live in fresh buffers
    third = backward(da2d.clone(), z1d.clone(), 0.0)
    assert torch.equal(third["dw"], outs["dw"]), "dw with the other outputs in fresh buffers"
    # the group-blocked operands [C / V][N H W][V]: saved by the forward kernel, and arriving blocked
    blk = lambda t: t.reshape(N * H * W, C // V, V).permute(1, 0, 2).contiguous().view(N, H, W, C)   # noqa: E731
    z1blk, z0blk = forward(z0d, "out")
    assert torch.equal(z1blk, blk(z1d)) and torch.equal(z0blk, blk(z0d))
    o2 = backward(da2d, z1blk, 1.0, z0_blocked=z0blk, z1_blocked=True)
    o3 = backward(blk(da2d), z1blk, 2.0, z0_blocked=z0blk, z1_blocked=True, da2_blocked=True)
    for name in outs:
        assert torch.equal(o2[name], outs[name]), "blocked layout: " + name
        assert torch.equal(o3[name], outs[name]), "blocked operands: " + name
