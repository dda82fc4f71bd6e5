"""A float64 parity case for every row-marching depthwise kernel instance (tests/dwmarch_instances.py: 60 template instances of
dwm_conv_k / dwm_bwd_s2_k behind mliis_dwconv_bn_fwd, mliis_dwconv_bn_bwd and mliis_mbconv_dw_bwd_march) at two kinds of shape: an
`edge` shape (bands with a narrower last one, several chunks of two steps, a channel tail) and a `long` shape whose single chunk
marches 5 to 9 steps, so that loads issued inside the pipeline's loop are consumed and the LDS ring comes round to a used slot --
which the shapes of test_dwmarch_gpu.py (at most two steps per chunk in test_dwmarch_shapes) and test_bf16_storage_gpu.py never do.

References are float64 torch on the CPU (oracle.efficientlab_ref.conv2d_same + autograd) on identically rounded operands: a tensor
that is bf16 on the device holds bf16-exact values in the reference, every other operand the fp32 value the device gets.  Bars are
the suite's: forward 2e-5, backward 1e-4, statistics 1e-5 of the tensor's max-abs (test_ops_gpu.close), one bf16 ulp for a bf16
tensor (test_bf16_storage_gpu.ulp_close).  Outputs are allocated full of NaN, so a pixel a step's mask drops fails the comparison
instead of reading as a stale zero; side buffers carry a sentinel behind the blocks the launch owns."""
import pytest
import torch

import dwmarch_instances as DI
from tests.test_bf16_storage_gpu import ulp_close
from tests.test_ops_gpu import dev

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(DI.target_overridden(), reason=DI.ENV_TARGET + " is set: the chunk counts are not the ones the cases were picked for")]

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
SENTINEL, SLACK = 7.0, 4096


def close(got, ref, tol, what=""):
    """test_ops_gpu.close, with the figure printed beside its bar (shown for a failing test, or with -s)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)
    print("{}: rel err {:.3e} (bar {:.1e})".format(what, err, tol))
    assert err <= tol, "{}: rel err {:.3e} > {:.1e}".format(what, err, tol)     # (a NaN fails: it is not <= tol)


def to_dev(t, ty, d):
    """A float64 tensor of DI.stored(., ty) values as the device tensor of that storage type (exact)."""
    return t.float().to(DT[ty]).contiguous().to(d)


def vec(t, d):
    return t.float().contiguous().to(d)


def f32x(t):
    return t.float().double()


def nan_out(shape, ty, d):
    return torch.full(shape, float("nan"), dtype=DT[ty], device=d)


def side_buffer(floats, d):
    """[floats of NaN the launch must overwrite][SLACK sentinels it must not touch]."""
    b = torch.full((floats + SLACK,), SENTINEL, device=d)
    b[:floats] = float("nan")
    return b


def check_tail(buf, floats, what):
    assert (buf[floats:] == SENTINEL).all().item(), what + ": written past its blocks"


def check_blocks(c, nb):
    N, H, W, C = c.shape
    from mliis_amd import ops
    g = DI.geom(c.inst, c.shape)
    q = ops.lib.raw("mliis_dwconv_bn_fwd_blocks" if c.inst.entry == "fwd" else "mliis_dwconv_bn_bwd_blocks")
    assert nb == g.blocks == N * g.bands * g.chunks == q(N, H, W, C, c.inst.k, c.inst.s), (nb, g)


def params(C, seed):
    """(w-independent) fp32-exact per-channel vectors: gamma, beta."""
    return f32x(1.0 + 0.2 * DI.rnd(C, seed=seed)), f32x(0.1 * DI.rnd(C, seed=seed + 1))


# ---------------------------------------------------------------------------------------------------------------- forward
def run_fwd(c):
    from mliis_amd import ops
    d = dev()
    i, (N, H, W, C) = c.inst, c.shape
    z = DI.stored(DI.rnd(N, H, W, C, seed=1, scale=1.5) + 0.3, i.ta)
    w = f32x(DI.rnd(i.k, i.k, C, 1, seed=2))
    gamma, beta = params(C, 3)
    mean, var, rstd = DI.batch_stats(z)
    a = DI.bn_swish(z, mean, rstd, gamma, beta)[0] if i.bn else z
    yr, _, _ = DI.conv_with_grads(a, w, i.s, lambda shape: None)

    zg, wg = to_dev(z, i.ta, d), vec(w, d)
    out = nan_out(tuple(yr.shape), i.tb, d)
    blocks = DI.geom(i, c.shape).blocks
    sp = side_buffer(blocks * 2 * C, d)
    if i.bn:
        # the producer's stage-1 sums in 5 uneven partial blocks, as test_dwmarch_gpu._case leaves them
        s1, s2 = z.sum(dim=(0, 1, 2)), (z * z).sum(dim=(0, 1, 2))
        cuts = torch.tensor([0.1, 0.35, 0.05, 0.3, 0.2], dtype=torch.float64)
        part0 = torch.stack([torch.stack([s1 * c_, s2 * c_]) for c_ in cuts]).float().contiguous().to(d)
        mm0, mv0 = f32x(0.2 * DI.rnd(C, seed=6)), f32x(1.0 + 0.1 * DI.rnd(C, seed=7).abs())
        mg, rg = nan_out((C,), "f32", d), nan_out((C,), "f32", d)
        mmg, mvg = vec(mm0, d), vec(mv0, d)
        y, nb = ops.dwconv_bn_fwd(zg, wg, i.s, bn=(vec(gamma, d), vec(beta, d), mg, rg, mmg, mvg), part=part0, nblk=5, out=out, stats_part=sp)
        close(mg, mean, 1e-5, "bn mean")
        close(rg, rstd, 1e-5, "bn rstd")
        close(mmg, mm0 - (mm0 - mean) * (1.0 - DI.MOM), 1e-5, "moving mean")
        close(mvg, mv0 - (mv0 - var) * (1.0 - DI.MOM), 1e-5, "moving variance")
    else:
        y, nb = ops.dwconv_bn_fwd(zg, wg, i.s, out=out, stats_part=sp)
    assert y is out and y.dtype == DT[i.tb]
    check_blocks(c, nb)
    if i.tb == "f32":
        close(y, yr, 2e-5, "y")
    else:
        ulp_close(y, yr.float(), "y")
    sums = sp[:nb * 2 * C].view(nb, 2, C).double().sum(0).cpu()
    if i.tb == "f32":
        ys, tol = yr, 1e-5                      # the values as stored (held to yr at 2e-5 above)
    elif i.k == 3:
        ys, tol = y.float().cpu().double(), 2e-5   # bf16 output: the sums see what the consumers will read back
    else:
        ys, tol = yr, 1e-5                      # 5x5 forward, bf16 output: sums of the unrounded accumulators (dwmarch.hip, compute())
    close(sums[0], ys.sum(dim=(0, 1, 2)), tol, "emitted sum")
    close(sums[1], (ys * ys).sum(dim=(0, 1, 2)), tol, "emitted sum of squares")
    check_tail(sp, nb * 2 * C, "statistics")


# ---------------------------------------------------------------------------------------------------------------- backward
def check_bwd(c, dx, dwp, bnp, nb, ga, gw, u0, xhat0):
    """dx, the filter-gradient slabs and (u0 given) bn0's stage-1 sums of a backward launch against the float64 gradients."""
    i, C = c.inst, c.shape[3]
    kk = i.k * i.k
    check_blocks(c, nb)
    if i.tb == "f32":
        close(dx, ga, 1e-4, "dx")
        dx_used = ga
    else:
        ulp_close(dx, ga.float(), "dx")
        dx_used = dx.float().cpu().double()      # the sums below are formed from the ROUNDED dx (dwm_stored): dx itself is held to the oracle above
    close(dwp[:nb * kk * C].view(nb, i.k, i.k, C).double().sum(0).cpu()[..., None], gw, 1e-4, "filter-gradient slabs")
    check_tail(dwp, nb * kk * C, "filter-gradient slabs")
    if u0 is not None:
        g = dx_used * DI.swish_grad(u0)
        sums = bnp[:nb * 2 * C].view(nb, 2, C).double().sum(0).cpu()
        close(sums[0], g.sum(dim=(0, 1, 2)), 1e-4, "bn0 stage 1: sum g")
        close(sums[1], (g * xhat0).sum(dim=(0, 1, 2)), 1e-4, "bn0 stage 1: sum g xhat")
        check_tail(bnp, nb * 2 * C, "bn0 stage 1")


def run_bwd(c):
    from mliis_amd import ops
    d = dev()
    i, (N, H, W, C) = c.inst, c.shape
    z = DI.stored(DI.rnd(N, H, W, C, seed=1, scale=1.5) + 0.3, i.tb)
    w = f32x(DI.rnd(i.k, i.k, C, 1, seed=2))
    gamma, beta = params(C, 3)
    mean, _, rstd = DI.batch_stats(z)
    mean, rstd = f32x(mean), f32x(rstd)          # given to the launch as fp32 vectors: the reference normalises with those
    a, u, xhat = DI.bn_swish(z, mean, rstd, gamma, beta) if i.bn else (z, None, None)
    held = {}

    def dy_of(shape):
        held["dy"] = DI.stored(DI.rnd(*shape, seed=5), i.ta)
        return held["dy"]
    _, ga, gw = DI.conv_with_grads(a, w, i.s, dy_of)

    blocks = DI.geom(i, c.shape).blocks
    dwp = side_buffer(blocks * i.k * i.k * C, d)
    bnp = side_buffer(blocks * 2 * C, d) if i.bn else None
    dx = nan_out((N, H, W, C), i.tb, d)
    bn = (vec(mean, d), vec(rstd, d), vec(gamma, d), vec(beta, d)) if i.bn else None
    got, none_, nb = ops.dwconv_bn_bwd(to_dev(held["dy"], i.ta, d), to_dev(z, i.tb, d), vec(w, d), i.s, bn=bn, out=dx, dw_part=dwp, bn_part=bnp)
    assert got is dx and none_ is None
    check_bwd(c, dx, dwp, bnp, nb, ga, gw, u, xhat)


def run_fused(c):
    from mliis_amd import ops
    d = dev()
    i, (N, H, W, C) = c.inst, c.shape
    Ho, Wo = -(-H // i.s), -(-W // i.s)
    z0 = DI.stored(DI.rnd(N, H, W, C, seed=1, scale=1.5) + 0.3, i.tb)
    z1 = DI.stored(DI.rnd(N, Ho, Wo, C, seed=2, scale=1.2) - 0.2, i.ta)
    da2 = DI.stored(DI.rnd(N, Ho, Wo, C, seed=3), i.ta)
    w = f32x(DI.rnd(i.k, i.k, C, 1, seed=4))
    gate, ca = f32x(torch.sigmoid(DI.rnd(N, C, seed=5))), f32x(0.01 * DI.rnd(N, C, seed=6))
    g0, b0 = params(C, 7)
    g1, b1 = params(C, 9)
    m0, _, r0 = (f32x(t) for t in DI.batch_stats(z0))
    m1, _, r1 = (f32x(t) for t in DI.batch_stats(z1))
    dz1, stage1, dga_ref, dbe_ref = DI.fused_dz1(da2, z1, m1, r1, g1, b1, gate, ca)
    a0, u0, xhat0 = DI.bn_swish(z0, m0, r0, g0, b0)
    _, ga, gw = DI.conv_with_grads(a0, w, i.s, lambda shape: dz1)

    blocks = DI.geom(i, c.shape).blocks
    dwp, bnp = side_buffer(blocks * i.k * i.k * C, d), side_buffer(blocks * 2 * C, d)
    dx = nan_out((N, H, W, C), i.tb, d)
    dga, dbe = nan_out((C,), "f32", d), nan_out((C,), "f32", d)
    nb = ops.mbconv_dw_bwd_march(to_dev(da2, i.ta, d), to_dev(z1, i.ta, d), (vec(m1, d), vec(r1, d), vec(g1, d), vec(b1, d)), vec(gate, d), vec(ca, d),
                                 stage1.contiguous().to(d), dga, dbe, to_dev(z0, i.tb, d), (vec(m0, d), vec(r0, d), vec(g0, d), vec(b0, d)), vec(w, d),
                                 i.s, dx, dwp, bnp)
    check_bwd(c, dx, dwp, bnp, nb, ga, gw, u0, xhat0)
    close(dga, dga_ref, 1e-5, "dgamma1")
    close(dbe, dbe_ref, 1e-5, "dbeta1")


RUN = {"fwd": run_fwd, "bwd": run_bwd, "fused": run_fused}


@pytest.mark.parametrize("case", DI.cases(), ids=DI.case_id)
def test_dwmarch_instance(case):
    RUN[case.inst.entry](case)

