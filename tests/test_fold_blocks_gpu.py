"""Block-count edges of the fold of a producer's partial batch-norm sums ([nblk][2][C], csrc/bn_fold.hpp): 256 threads = 8 channel
quads x 32 fold lanes, each lane takes blocks lane, lane + 32, ... in rounds of 8 (fold32; dwm_bn_begin / dwm_bn_end of dwmarch.hip
issue the same rounds and leave the last one in flight under the kernel's own loads), surplus slots re-read a valid block and are
masked.  The other tests hand over 5 partials, or what bn_stats_partial leaves for their shape; here nblk runs over

    1, 31          lanes without a block            32, 33      every lane one block / one lane two
    255, 256, 257  the round boundary (32 x 8)      288, 289    a second round of one block per lane / one lane two
    545            two full rounds and a tail

for the consumers ops.dwconv_bn_fwd (3x3 stride 1, 5x5 stride 2), ops.bn_apply_fused (post-swish) and ops.mbconv_dw_fwd_small.

The float64 stage-1 sums of z are cut into nblk uneven positive shares and cast to fp32; the reference statistics come from the
float64 sum of those fp32 shares.  The partial buffer is exactly nblk * 2 * C floats at the head of a larger allocation whose tail is
NaN: a surplus slot that is summed (not merely re-read from a valid block) shows as NaN.  mean / rstd at 1e-5, the output at 2e-5 of
its max-abs against the float64 computation with the reference statistics (test_ops_gpu.close)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import efficientlab_ref as R  # noqa: E402
from tests.test_ops_gpu import close, dev, nchw, nhwc, rnd  # noqa: E402

EPS = 1e-3
NBLK = (1, 31, 32, 33, 255, 256, 257, 288, 289, 545)
SHAPE = (2, 9, 10, 36)
SMALL_SHAPE = (8, 14, 14, 40)     # mliis_mbconv_dw_small_supported


def f32x(t):
    return t.float().double()


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """(z, gamma, beta) in float64 holding fp32 values; shared by the cases and left unchanged."""
    C = shape[3]
    return f32x(rnd(*shape, seed=1, scale=1.5) + 0.3), f32x(1.0 + 0.2 * rnd(C, seed=2)), f32x(0.1 * rnd(C, seed=3))


def partials(z, nblk, d):
    """(part, mean, rstd): part = nblk * 2 * C floats in front of a NaN tail; mean / rstd from the float64 sum of the fp32 shares."""
    C = z.shape[3]
    rows = z.shape[0] * z.shape[1] * z.shape[2]
    tot = torch.stack([z.sum(dim=(0, 1, 2)), (z * z).sum(dim=(0, 1, 2))])                        # [2, C]
    share = 0.25 + torch.rand(nblk, generator=torch.Generator().manual_seed(100 + nblk), dtype=torch.float64)
    share = share / share.sum()                                                                   # uneven, positive
    blocks = (share[:, None, None] * tot[None]).float()                                           # [nblk, 2, C] as a producer leaves them
    s = blocks.double().sum(0)
    mean = s[0] / rows
    rstd = 1.0 / torch.sqrt((s[1] / rows - mean * mean).clamp_min(0.0) + EPS)
    buf = torch.full((nblk * 2 * C + 8 * 2 * C + 64,), float("nan"), device=d)
    buf[:nblk * 2 * C] = blocks.reshape(-1).to(d)
    return buf[:nblk * 2 * C], mean, rstd


def act(z, mean, rstd, gamma, beta):
    u = (z - mean) * rstd * gamma + beta
    return u * torch.sigmoid(u)


def stat_outputs(C, d):
    return torch.full((C,), float("nan"), device=d), torch.full((C,), float("nan"), device=d)


@pytest.mark.parametrize("nblk", NBLK)
@pytest.mark.parametrize("k,s", [(3, 1), (5, 2)])
def test_marching_depthwise_forward_folds_any_block_count(k, s, nblk):
    from mliis_amd import ops
    d = dev()
    z, gamma, beta = inputs(SHAPE)
    C = SHAPE[3]
    w = f32x(rnd(k, k, C, 1, seed=4))
    part, mean, rstd = partials(z, nblk, d)
    mg, rg = stat_outputs(C, d)
    y = torch.full((SHAPE[0], -(-SHAPE[1] // s), -(-SHAPE[2] // s), C), float("nan"), device=d)
    ops.dwconv_bn_fwd(z.float().to(d), w.float().to(d), s, bn=(gamma.float().to(d), beta.float().to(d), mg, rg, None, None), part=part, nblk=nblk, out=y)
    close(mg, mean, 1e-5, "mean")
    close(rg, rstd, 1e-5, "rstd")
    close(y, nhwc(R.conv2d_same(nchw(act(z, mean, rstd, gamma, beta)), w, s, groups=C)), 2e-5, "y")


@pytest.mark.parametrize("nblk", NBLK)
def test_bn_apply_fused_folds_any_block_count(nblk):
    from mliis_amd import ops
    d = dev()
    z, gamma, beta = inputs(SHAPE)
    C = SHAPE[3]
    part, mean, rstd = partials(z, nblk, d)
    mg, rg = stat_outputs(C, d)
    y = torch.full(SHAPE, float("nan"), device=d)
    ops.bn_apply_fused(z.float().to(d), part, nblk, mg, rg, gamma.float().to(d), beta.float().to(d), post_swish=True, out=y)
    close(mg, mean, 1e-5, "mean")
    close(rg, rstd, 1e-5, "rstd")
    close(y, act(z, mean, rstd, gamma, beta), 2e-5, "y")


@pytest.mark.parametrize("nblk", NBLK)
def test_small_map_mbconv_forward_folds_any_block_count(nblk):
    from mliis_amd import ops
    d = dev()
    N, H, W, C = SMALL_SHAPE
    k = 3
    assert ops.mbconv_dw_small_supported(N, H, W, C, k, 1)
    z0, g0, b0 = inputs(SMALL_SHAPE)
    w = f32x(rnd(k, k, C, 1, seed=4))
    g1, b1 = f32x(1.0 + 0.2 * rnd(C, seed=5)), f32x(0.1 * rnd(C, seed=6))
    part, mean0, rstd0 = partials(z0, nblk, d)
    m0, r0 = stat_outputs(C, d)
    m1, r1 = stat_outputs(C, d)
    z1, a1 = torch.full(SMALL_SHAPE, float("nan"), device=d), torch.full(SMALL_SHAPE, float("nan"), device=d)
    s = torch.full((N, C), float("nan"), device=d)
    v = lambda t: t.float().to(d)  # noqa: E731
    ops.mbconv_dw_fwd_small(v(z0), part, nblk, (v(g0), v(b0), m0, r0, None, None), v(w), (v(g1), v(b1), m1, r1, None, None), z1, a1, s)
    close(m0, mean0, 1e-5, "mean0")
    close(r0, rstd0, 1e-5, "rstd0")
    z1r = nhwc(R.conv2d_same(nchw(act(z0, mean0, rstd0, g0, b0)), w, 1, groups=C))
    close(z1, z1r, 2e-5, "z1")     # (bn1's statistics, a1 and the pooled means follow from z1: test_ops_gpu.py holds them to the oracle)
