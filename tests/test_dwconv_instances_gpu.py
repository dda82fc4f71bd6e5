"""A float64 parity case for every plain-depthwise kernel instance a call below 2 GiB can launch (tests/dwconv_instances.py: 21 of the
31 template instances behind mliis_dwconv_fwd, mliis_dwconv_bwd_data, mliis_dwconv_bwd_data_bn and mliis_dwconv_bwd_filter), at the
shapes and buffer sizes where the launchers change route and the kernels have their tails: ragged tiles on both axes with a channel
tail, maps smaller than the filter, stride-2 maps of even, odd and mixed parity, a statistics buffer that fits one layout but not the
other, a stage-1 buffer one float short (the fallback that reports 0 blocks), and for the filter gradient idle lanes, a partial
channel group, a partial last block and a walk of two strips.

The reference is oracle.efficientlab_ref.conv2d_same with autograd in float64 on seeded, fp32-exact inputs, computed once per
(k, stride, shape).  Bars are the suite's (test_ops_gpu.close, relative to the tensor's max-abs): forward 2e-5, dx and dw 1e-4,
statistics sums 1e-5, batch-norm stage-1 quantities 2e-4.  Every call writes into outputs full of NaN and into side buffers whose
owned extent is NaN and whose rest is a sentinel, then runs again into buffers with another fill and must give the same bits; the
block count the library reports must be the mirror's.

Worst figures seen on an MI355X over all cases, for information (bar in brackets):
  forward          y 1.7e-7 (2e-5); sum y 1.7e-7, sum y^2 1.4e-7 (1e-5); sliding-window y against tile y: the same bits
  backward data    dx 1.6e-7 (1e-4)
  ... with bn      dx 2.0e-7 (1e-4), against the plain call 1.2e-7 (1e-6), the fallbacks the same bits for k = 3 and k = 5;
                   sum g 1.3e-7, sum g xhat 1.8e-7 (2e-4); bn_bwd from them dx 2.3e-7, dgamma 1.9e-7, dbeta 1.6e-7 (2e-4)
  backward filter  dw 1.2e-7, float64 sum of the slabs 1.2e-7 (1e-4); the library's fold of the slabs, redone on the host: the same bits
"""
import functools

import pytest
import torch

import dwconv_instances as DI

pytestmark = pytest.mark.gpu

from oracle import efficientlab_ref as R  # noqa: E402
from test_ops_gpu import close, dev, f32, nchw, nhwc, rnd  # noqa: E402

NAN, SLACK = float("nan"), 4096
FILLS = ((NAN, 7.0), (-3.0, 5.0))          # (outputs and owned extents, sentinel behind them) of the first and the second run


def check(got, ref, tol, what):
    """test_ops_gpu.close with the figure printed beside its bar (shown for a failing test, or with -s).  close() measures against the
    largest entry of the reference, and no vector of column sums here is near zero as a whole -- but for the one-row batch norm's
    sum g xhat, an exact zero on both sides -- so none needs the scale of its terms' absolute values instead."""
    g, r = got.detach().cpu().double(), ref.detach().cpu().double()
    err = (g - r).abs().max().item() / max(r.abs().max().item(), 1e-30) if g.shape == r.shape else NAN
    print("dwconv-figure | {} | {:.3e} | {:.1e}".format(what, err, tol))
    close(got, ref, tol, what)


def fp32_exact(t):
    return t.float().double()


def out_of(shape, fill, d):
    return torch.full(tuple(shape), fill, device=d)


def side_buffer(floats, extent, fills, d):
    """[extent floats the launch must overwrite][the rest of `floats` and SLACK more it must not touch]."""
    b = torch.full((floats + SLACK,), fills[1], device=d)
    b[:extent] = fills[0]
    return b


def check_side_buffer(buf, extent, fills, what):
    assert (buf[extent:] == fills[1]).all().item(), what + ": written past its extent"
    assert torch.isfinite(buf[:extent]).all().item(), what + ": a float of its extent not written"


def same_bits(a, b, what):
    for x, y in zip(a, b):
        assert torch.equal(x, y), what + ": a second call into other buffers gave other bits"


# ---------------------------------------------------------------------------------------------------------------- references
@functools.lru_cache(maxsize=None)
def _oracle(k, s, shape):
    """Inputs and float64 results of one layer; computed once per (k, stride, shape), shared by the entry points, never written."""
    N, H, W, C = shape
    x = fp32_exact(rnd(N, H, W, C, seed=1)).requires_grad_(True)
    w = fp32_exact(rnd(k, k, C, 1, seed=2, scale=0.4)).requires_grad_(True)
    y = R.conv2d_same(nchw(x), w, s, groups=C)
    dy = fp32_exact(rnd(*y.shape, seed=3))
    gx, gw = torch.autograd.grad(y, [x, w], dy)
    return dict(x=x.detach(), w=w.detach(), y=nhwc(y.detach()), dy=nhwc(dy), gx=gx.detach(), gw=gw.detach())


@functools.lru_cache(maxsize=None)
def _oracle_bn(k, s, shape):
    """The depthwise conv behind a = swish(bn(z)) with batch statistics, as in test_dwconv_bwd_data_emits_bn_backward_stage1: the
    gradients w.r.t. a (the conv alone), z, gamma and beta; dbeta = sum g and dgamma = sum g xhat, g = da * swish'(gamma xhat + beta), are
    what stage 1 adds up."""
    N, H, W, C = shape
    z = fp32_exact(rnd(N, H, W, C, seed=100)).requires_grad_(True)
    gamma = fp32_exact(rnd(C, seed=101) * 0.3 + 1.0).requires_grad_(True)
    beta = fp32_exact(rnd(C, seed=102) * 0.2).requires_grad_(True)
    w = fp32_exact(rnd(k, k, C, 1, seed=103, scale=0.3))
    mean = z.mean(dim=(0, 1, 2))
    var = ((z - mean) ** 2).mean(dim=(0, 1, 2))
    rstd = 1.0 / torch.sqrt(var + 1e-3)
    xhat = (z - mean) * rstd
    u = xhat * gamma + beta
    a = R.swish(u)
    y = R.conv2d_same(nchw(a), w, s, groups=C)
    dy = fp32_exact(rnd(*y.shape, seed=104))
    ga, gz, gg, gb = (t.detach() for t in torch.autograd.grad(y, [a, z, gamma, beta], dy))
    return dict(z=z.detach(), gamma=gamma.detach(), beta=beta.detach(), w=w, mean=mean.detach(), rstd=rstd.detach(), dy=nhwc(dy), ga=ga, gz=gz,
                gg=gg, gb=gb)


def cases_of(entry):
    return [c for c in DI.cases() if DI.entry_of(c) == entry]


# ---------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("c", cases_of("fwd"), ids=DI.case_id)
def test_forward(c):
    from mliis_amd import ops
    d = dev()
    o = _oracle(c.k, c.s, c.shape)
    N, H, W, C = c.shape
    xg, wg = f32(o["x"], d), f32(o["w"], d)
    inst, blocks = DI.launched(c)
    assert inst == c.inst
    extent = blocks * 2 * C

    def run(fills):
        y = out_of(o["y"].shape, fills[0], d)
        if c.floats is None:
            assert ops.dwconv_fwd(xg, wg, c.s, out=y) is y
            return (y,)
        buf = side_buffer(c.floats, extent, fills, d)
        _, nblk = ops.dwconv_fwd(xg, wg, c.s, out=y, stats_part=buf[:c.floats])
        assert nblk == blocks, "route: {} blocks reported, {} predicted for {}".format(nblk, blocks, DI.kernel_name(inst))
        check_side_buffer(buf, extent, fills, "statistics")
        return y, buf[:extent].clone()

    first = run(FILLS[0])
    y = first[0]
    assert torch.isfinite(y).all().item()
    check(y, o["y"], 2e-5, "fwd y")
    if c.floats is not None:
        # the same output as the call without statistics: the same bits where both run the same kernel family
        plain = ops.dwconv_fwd(xg, wg, c.s, out=out_of(o["y"].shape, NAN, d))
        if (inst.kernel == "tile") == (DI.fwd_route(N, H, W, C, c.k, c.s, None)[0].kernel == "tile"):
            assert torch.equal(y, plain), "y with statistics != y without"
        else:
            check(y, plain, 2e-5, "fwd y (sliding window) vs y (tile)")
        sums = first[1].view(blocks, 2, C).double().sum(0).cpu()
        check(sums[0], o["y"].sum(dim=(0, 1, 2)), 1e-5, "fwd sum y")
        check(sums[1], (o["y"] * o["y"]).sum(dim=(0, 1, 2)), 1e-5, "fwd sum y^2")
    same_bits(first, run(FILLS[1]), "forward")


# ---------------------------------------------------------------------------------------------------------------- backward data
@pytest.mark.parametrize("c", cases_of("bwd_data"), ids=DI.case_id)
def test_backward_data(c):
    from mliis_amd import ops
    d = dev()
    o = _oracle(c.k, c.s, c.shape)
    N, H, W, C = c.shape
    dyg, wg = f32(o["dy"], d), f32(o["w"], d)
    assert DI.launched(c) == (c.inst, 0)

    def run(fills):
        dx = out_of(c.shape, fills[0], d)
        assert ops.dwconv_bwd_data(dyg, wg, c.s, (H, W), out=dx) is dx
        return (dx,)

    first = run(FILLS[0])
    assert torch.isfinite(first[0]).all().item()
    check(first[0], o["gx"], 1e-4, "bwd_data dx")
    same_bits(first, run(FILLS[1]), "backward data")


@pytest.mark.parametrize("c", cases_of("bwd_data_bn"), ids=DI.case_id)
def test_backward_data_with_batch_norm_sums(c):
    from mliis_amd import ops
    d = dev()
    o = _oracle_bn(c.k, c.s, c.shape)
    N, H, W, C = c.shape
    dyg, wg, zg = f32(o["dy"], d), f32(o["w"], d), f32(o["z"], d)
    stats = tuple(f32(o[n], d) for n in ("mean", "rstd", "gamma", "beta"))
    inst, blocks = DI.launched(c)
    fallback = c.kind == "fallback"
    assert (blocks == 0) == fallback and (fallback or inst == c.inst)
    extent = blocks * 2 * C
    one_row = N * H * W == 1          # mliis_bn_bwd takes rows > 1: the 1 x 1 map checks the conv's own outputs only

    def run(fills):
        da = out_of(c.shape, fills[0], d)
        buf = side_buffer(c.floats, extent, fills, d)
        _, nblk = ops.dwconv_bwd_data(dyg, wg, c.s, (H, W), out=da, bn=(zg,) + stats, part=buf[:c.floats])
        assert nblk == blocks, "route: {} blocks reported, {} predicted for {}".format(nblk, blocks, DI.kernel_name(inst))
        check_side_buffer(buf, extent, fills, "stage 1")          # (fallback: extent 0 -- the whole buffer still holds the sentinel)
        if one_row:
            return [da, buf[:extent].clone()]
        outs = [out_of(c.shape, fills[0], d), out_of((C,), fills[0], d), out_of((C,), fills[0], d)]
        ops.bn_bwd(zg, da, *stats, False, True, dx=outs[0], dgamma=outs[1], dbeta=outs[2], stage1=None if fallback else (buf[:c.floats], nblk))
        return [da, buf[:extent].clone()] + outs

    first = run(FILLS[0])
    da, part = first[:2]
    assert all(torch.isfinite(t).all().item() for t in first)
    check(da, o["ga"], 1e-4, "bwd_data_bn dx")
    plain = ops.dwconv_bwd_data(dyg, wg, c.s, (H, W), out=out_of(c.shape, NAN, d))
    if fallback:
        if c.k == 5:        # both calls run the unfused tile kernel
            assert torch.equal(da, plain), "fallback dx != plain dx"
        else:
            check(da, plain, 1e-6, "bwd_data_bn fallback dx vs plain dx")
    else:
        check(da, plain, 1e-6, "bwd_data_bn dx vs plain dx")
        sums = part.view(blocks, 2, C).double().sum(0).cpu()
        check(sums[0], o["gb"], 2e-4, "bwd_data_bn sum g vs dbeta")
        check(sums[1], o["gg"], 2e-4, "bwd_data_bn sum g xhat vs dgamma")
    if not one_row:
        dz, dgamma, dbeta = first[2:]
        tag = "bn_bwd (own reduce pass) " if fallback else "bn_bwd (stage 1 from the conv) "
        check(dz, o["gz"], 2e-4, tag + "dx")
        check(dgamma, o["gg"], 2e-4, tag + "dgamma")
        check(dbeta, o["gb"], 2e-4, tag + "dbeta")
    same_bits(first, run(FILLS[1]), "backward data with the batch-norm sums")


# ---------------------------------------------------------------------------------------------------------------- backward filter
def fold_like_the_library(slabs):
    """fold_flat_k: 16 lanes stride over the slabs adding in double, the lanes are added in order, the sum is rounded to fp32."""
    s = slabs.cpu().double()
    lanes = []
    for y in range(16):
        acc = torch.zeros(s.shape[1], dtype=torch.float64)
        for b in range(y, s.shape[0], 16):
            acc = acc + s[b]
        lanes.append(acc)
    r = torch.zeros(s.shape[1], dtype=torch.float64)
    for acc in lanes:
        r = r + acc
    return r.float()


@pytest.mark.parametrize("c", cases_of("bwd_filter"), ids=DI.case_id)
def test_backward_filter(c):
    from mliis_amd import ops
    d = dev()
    o = _oracle(c.k, c.s, c.shape)
    N, H, W, C = c.shape
    k = c.k
    xg, dyg = f32(o["x"], d), f32(o["dy"], d)
    nblk = DI.filter_geom(N, H, W, C, k, c.s).nblk
    assert c.floats == nblk * k * k * C == ops.dwconv_bwd_filter_floats(N, H, W, C, k, c.s)

    def run(fills):
        dw = out_of((k, k, C, 1), fills[0], d)
        ws = ops.Workspace(d, floats=c.floats + SLACK)
        ws.buf.fill_(fills[1])
        ws.buf[:c.floats] = fills[0]
        assert ops.dwconv_bwd_filter(xg, dyg, k, c.s, out=dw, ws=ws) is dw
        check_side_buffer(ws.buf, c.floats, fills, "workspace")
        slab = side_buffer(c.floats, c.floats, fills, d)
        ops.dwconv_bwd_filter(xg, dyg, k, c.s, partial=slab[:c.floats])          # dw == NULL: the slabs stay where they are
        check_side_buffer(slab, c.floats, fills, "slabs")
        assert torch.equal(slab[:c.floats], ws.buf[:c.floats]), "slab mode wrote other slabs than the folded call"
        return dw, slab[:c.floats].clone()

    first = run(FILLS[0])
    dw, slabs = first
    assert torch.isfinite(dw).all().item()
    check(dw, o["gw"], 1e-4, "bwd_filter dw")
    slabs = slabs.view(nblk, k * k * C)
    check(slabs.double().sum(0).view(k, k, C, 1), o["gw"], 1e-4, "bwd_filter float64 sum of the slabs")
    assert torch.equal(fold_like_the_library(slabs), dw.cpu().view(-1)), "the fold of the slabs is not what the folded call returned"
    same_bits(first, run(FILLS[1]), "backward filter")
