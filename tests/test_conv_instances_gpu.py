"""A parity case for every dense-conv kernel instance the planners can pick (tests/conv_instances.py): each test takes one kernel
family and one operand precision, asks the planner queries for the cheapest shape with a row, K and column tail that launches each
instance, asserts the name query before every launch and compares with the float64 result of the identically rounded operands.
Tolerances are test_ops_gpu.py's: forward 2e-5, backward 1e-4 of the tensor's max-abs, 2e-4 for an fp8 forward (the fp8 MFMA aligns
the 32 products of a K block before adding).  A test passes only if the set of names it launched is the declared set of its family
and precision without the UNREACHABLE entries -- no instance is skipped silently.

The seeded N(0,1) inputs are drawn on the device and copied to the host, the matrix products of the references run on the host in
float64 (`x.reshape(-1, K) @ w`, R.conv2d_same, autograd); their element-wise tails -- bias, swish, column sums, the comparison
itself -- run in float64 on the device, where the 66049-row maps of the 128-row-tile instances cost nothing."""
import contextlib
import functools
import math
import zlib

import pytest
import torch

import conv_instances as CI
from oracle import efficientlab_ref as R

pytestmark = pytest.mark.gpu

FWD_TOL = {"fp32": 2e-5, "bf16": 2e-5, "fp8": 2e-4}
SUM_TOL = {"fp32": 2e-5, "bf16": 2e-5, "fp8": 2e-4}   # (test_conv1x1_fp8_operands: the sums of an fp8 output at the output's own bar)
BWD_TOL = 1e-4
AIN_TOL = {"fp32": 2e-5, "bf16": 1e-2, "fp8": 1e-1}   # test_conv1x1_with_the_batch_norm_in_front_applied_on_load: against the UNROUNDED composition


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=4)
def _gen(shape, seed):
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    return torch.randn(*shape, generator=g, device="cuda:0", dtype=torch.float32)


def gen(*shape, seed, scale=1.0):
    """Seeded N(0, scale^2) fp32 tensor on the device (a fresh tensor: the cache keeps the draw)."""
    return _gen(tuple(shape), seed) * scale


def close(got, ref, tol, what=""):
    ref = ref.detach().to(device=got.device, dtype=torch.float64)
    got = got.detach().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    den = max(ref.abs().max().item(), 1e-30)
    err = (got - ref).abs().max().item() / den
    print("{}: rel err {:.3e} (bar {:.1e})".format(what, err, tol))   # (shown for a failing test, or with -s: the figures beside the bars)
    assert err <= tol, "{}: rel err {:.3e} > {:.1e}".format(what, err, tol)


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.fixture(scope="module")
def table():
    """instance name -> (shape, precision), searched on this device (its CU count decides the plans)."""
    dev()
    return CI.reached()


def expected(family, prec, table):
    want = CI.declared(family, prec) - set(CI.UNREACHABLE)
    assert {n for n, _ in CI.cases(family, prec, table)} == want, (family, prec)
    return want


def seed_of(s):
    return zlib.crc32(repr(tuple(s)).encode()) & 0xffff


def rounded(t32, rule, w=False):
    """fp32 operand -> float64 host tensor of what the matrix cores multiply."""
    t32 = t32.cpu()
    if rule == "none":
        return t32.double()
    if rule == "bf16":
        return t32.to(torch.bfloat16).double()          # round to nearest even, like v_cvt_pk_bf16_f32
    assert rule == "fp8"
    return R.round_fp8(t32, R.fp8_weight_scale(t32) if w else R.FP8_ACT_SCALE).double()


@contextlib.contextmanager
def every_case(failed):
    """A mismatch of one instance is recorded and the loop goes on, so that a failing test names every instance that is wrong (an error
    of another kind -- a failed launch, a fault -- ends the test at once)."""
    try:
        yield
    except AssertionError as e:
        failed.append(str(e).splitlines()[0])


def test_on_this_device_every_declared_instance_is_reached_or_has_a_reason(table):
    declared, hit, never = CI.all_declared(), set(table), set(CI.UNREACHABLE)
    assert hit <= declared and not (hit & never) and hit | never == declared, (sorted(hit - declared), sorted(hit & never), sorted(declared - hit - never))
    for fam, precs in CI.FAMILIES.items():
        for p in precs:
            expected(fam, p, table)


# ------------------------------------------------------------------------------------------------ forward and backward-data
def _stats_check(part, nblk, Nout, v, tol, what):
    assert nblk > 0, what
    sums = part[: nblk * 2 * Nout].view(nblk, 2, Nout).double().sum(0)
    close(sums[0], v.sum(dim=(0, 1, 2)), tol, what + ": fused sum")
    close(sums[1], (v * v).sum(dim=(0, 1, 2)), tol, what + ": fused sum of squares")
    assert (part[nblk * 2 * Nout:] == 7).all(), what + ": partial buffer's tail"


def _conv_case(name, s, prec, rule, gated, launched):
    from mliis_amd import ops
    d = dev()
    N, H, W, K, Nout, k = s.N, s.H, s.W, s.K, s.Nout, s.ksize
    sd = seed_of(s._replace(Nout=0, scale=False))   # (the instances of one map and K share the activations)
    dil = 2 if (k == 3 and min(H, W) >= 5 and sd % 2) else 1
    what = "{} {} gate={}".format(name, tuple(s), gated)
    xg = gen(N, H, W, K, seed=sd)
    wg = gen(k, k, K, Nout, seed=sd + 1, scale=1.0 / math.sqrt(k * k * K))
    bg = gen(Nout, seed=sd + 2)
    gg = torch.sigmoid(gen(N, K, seed=sd + 3)) if gated else None
    if rule == "fp8":
        xg[0, 0, 0, 0] = 40.0                                       # beyond 448 / 16: saturates
        if gated:
            gg[0, 0] = 1.0
    xs = xg * gg[:, None, None, :] if gated else xg                 # (the product multiplies in fp32, then converts)
    xq, wq = rounded(xs, rule), rounded(wg, rule, w=True)
    if k == 1:
        y = (xq.reshape(-1, K) @ wq.reshape(K, Nout)).reshape(N, H, W, Nout)
    else:
        y = nhwc(R.conv2d_same(nchw(xq), wq, 1, dil))
    y, b = y.to(d), bg.double()
    wt = ops.hwoi(wg)
    nst = (-(-N * H * W // 16)) * 2 * Nout + 64
    # plain; with bias and the fused statistics; with bias and the statistics of swish(value)
    for bias, stats, swish in ((False, False, False), (True, True, False), (True, True, True)):
        out = torch.full((N, H, W, Nout + 12), 5.0, device=d)
        part = torch.full((nst,), 7.0, device=d) if stats else None
        assert ops.conv2d_kernel_name(N, H, W, K, Nout, k, gated, prec) == name, what
        launched.add(name)
        r = ops.conv2d_fwd(xg, wg, bg if bias else None, dil, out=out[..., 8:8 + Nout], stats_part=part, stats_swish=swish, wt=wt, x_scale=gg,
                           precision=prec)
        ref = y + b if bias else y
        close(out[..., 8:8 + Nout], ref, FWD_TOL[prec], what + " fwd bias={} stats={} swish={}".format(bias, stats, swish))
        assert (out[..., :8] == 5).all() and (out[..., 8 + Nout:] == 5).all(), what + ": columns beside the output slice"
        if stats:
            _stats_check(part, r[1], Nout, R.swish(ref) if swish else ref, SUM_TOL[prec], what + " swish={}".format(swish))
    # backward-data of a 1x1 conv whose Cout is this K: dx = dy . W^T, the same GEMM and the same instance (an fp8-mode backward call
    # takes bf16 operands, i.e. the bf16 instance, which the bf16 case launches; the gate is a forward operand)
    if k == 1 and not gated and rule != "fp8":
        dyg = gen(N, H, W, K, seed=sd + 4)
        w2 = gen(1, 1, Nout, K, seed=sd + 5, scale=1.0 / math.sqrt(K))
        refx = (rounded(dyg, rule).reshape(-1, K) @ rounded(w2, rule).reshape(Nout, K).T).reshape(N, H, W, Nout)
        dx = torch.full((N, H, W, Nout + 4), -2.0, device=d)
        assert ops.conv2d_kernel_name(N, H, W, K, Nout, 1, False, prec) == name, what
        ops.conv2d_bwd_data(dyg, w2, 1, out=dx[..., :Nout], precision=prec)
        close(dx[..., :Nout], refx, BWD_TOL, what + " bwd data")
        assert (dx[..., Nout:] == -2).all(), what + ": columns beside the gradient slice"


@pytest.mark.parametrize("family,prec", [(f, p) for f in ("stream", "ksplit", "gemm", "sk") for p in CI.FAMILIES[f]])
def test_every_instance_forward_and_backward_data(family, prec, table):
    """Forward -- plain, with bias and the fused BN statistics, with the statistics of swish(value) -- into a channel slice of a
    sentinel-filled buffer, and for the 1x1 shapes backward-data with K in the role of Cout.  The GEMM's x_scale forms are instances
    of their own; conv1x1_ksplit_k takes the gate at run time and runs with and without it."""
    from mliis_amd import ops
    want = expected(family, prec, table)
    launched, failed = set(), []
    for name, s in sorted(CI.cases(family, prec, table), key=lambda c: (c[1].N, c[1].H, c[1].W, c[1].K, c[1].ksize, c[0])):
        gates = [s.scale]
        if family == "ksplit" and ops.conv2d_kernel_name(s.N, s.H, s.W, s.K, s.Nout, 1, not s.scale, prec) == name:   # (maps below 16 pixels: gated -> GEMM)
            gates.append(not s.scale)
        for gated in gates:
            with every_case(failed):
                _conv_case(name, s, prec, CI.ROUNDING[family][prec], gated, launched)
    assert not failed, "\n".join(failed)
    assert launched == want, (sorted(want - launched), sorted(launched - want))


# ------------------------------------------------------------------------------------------------ batch norm on load (AIN = true)
@pytest.mark.parametrize("prec", CI.FAMILIES["stream_ain"])
def test_every_stream_instance_with_the_batch_norm_on_load(prec, table):
    """mliis_conv2d_fwd_bnin at the shape of every reachable conv1x1_stream_k<..., AIN = true>: the float64 composition batch norm ->
    image scale -> residual -> 1x1 conv at the bars of test_conv1x1_with_the_batch_norm_in_front_applied_on_load, and -- the
    instance rounds the very tensor it writes to a_out -- the conv of those values, rounded, at the forward bar of every instance."""
    dev()
    want = expected("stream_ain", prec, table)
    rule = CI.ROUNDING["stream_ain"][prec]
    launched, failed = set(), []
    for name, s in CI.cases("stream_ain", prec, table):
        with every_case(failed):
            _ain_case(name, s, prec, rule, launched)
    assert not failed, "\n".join(failed)
    assert launched == want, (sorted(want - launched), sorted(launched - want))


def _ain_case(name, s, prec, rule, launched):
    from mliis_amd import ops
    d = dev()
    N, H, W, K, Nout = s.N, s.H, s.W, s.K, s.Nout
    sd = seed_of(s)
    zg = (gen(N, H, W, K, seed=sd) * (gen(K, seed=sd + 1).abs() + 0.5) + gen(K, seed=sd + 2)).contiguous()
    wg = gen(1, 1, K, Nout, seed=sd + 3, scale=1.0 / math.sqrt(K))
    gamma, beta, res = gen(K, seed=sd + 4) * 0.3 + 1, gen(K, seed=sd + 5), gen(N, H, W, K, seed=sd + 6)
    sc = (torch.rand(N, generator=torch.Generator().manual_seed(sd + 7)) > 0.3).float() / 0.7
    sc[0] = 1.0 / 0.7
    z = zg.cpu().double()
    mean, var = z.mean(dim=(0, 1, 2)), z.var(dim=(0, 1, 2), unbiased=False)
    a = ((z - mean) * torch.rsqrt(var + 1e-3) * gamma.cpu().double() + beta.cpu().double()) * sc.double()[:, None, None, None] + res.cpu().double()
    y = (a.reshape(-1, K) @ wg.cpu().double().reshape(K, Nout)).reshape(N, H, W, Nout)
    part = torch.full((1 << 20,), float("nan"), device=d)
    nblk = ops.bn_stats_partial(zg, False, part)
    m_o, r_o = torch.empty(K, device=d), torch.empty(K, device=d)
    a_out = torch.full((N, H, W, K), float("nan"), device=d)
    out = torch.full((N, H, W, Nout + 12), 5.0, device=d)
    nst = (-(-N * H * W // 16)) * 2 * Nout + 64
    spart = torch.full((nst,), 7.0, device=d)
    assert ops.conv2d_fwd_bnin_ok(N, H, W, K, Nout) and ops.conv2d_kernel_name(N, H, W, K, Nout, 1, False, prec)[:-1] + ", true>" == name
    launched.add(name)
    _, nb = ops.conv2d_fwd_bnin(zg, part, nblk, m_o, r_o, gamma, beta, a_out, wg, out[..., 8:8 + Nout], img_scale=sc.to(d), res=res,
                                stats_part=spart, precision=prec)
    close(a_out, a, 3e-5, name + " block tensor")
    close(m_o, mean, 1e-5, name + " mean")
    close(r_o, torch.rsqrt(var + 1e-3), 1e-5, name + " rstd")
    close(out[..., 8:8 + Nout], y, AIN_TOL[prec], name + " conv of the normalised tensor")
    assert (out[..., :8] == 5).all() and (out[..., 8 + Nout:] == 5).all(), name
    y2 = (rounded(a_out, rule).reshape(-1, K) @ rounded(wg, rule, w=True).reshape(K, Nout)).reshape(N, H, W, Nout).to(d)
    close(out[..., 8:8 + Nout], y2, FWD_TOL[prec], name + " conv of the rounded block tensor")
    _stats_check(spart, nb, Nout, y2, SUM_TOL[prec], name)


# ------------------------------------------------------------------------------------------------ filter gradients
@pytest.mark.parametrize("prec", CI.FAMILIES["filter"])
def test_every_filter_gradient_instance(prec, table):
    """mliis_conv2d_bwd_filter for every (TMF, NT, multitap, x_scale) plan_filter can give, against float64 autograd of the rounded
    operands (with an x_scale: of the rounded fp32 product x * x_scale)."""
    dev()
    want = expected("filter", prec, table)
    rule = CI.ROUNDING["filter"][prec]
    launched, failed = set(), []
    for name, s in sorted(CI.cases("filter", prec, table), key=lambda c: (tuple(c[1]._replace(scale=False)), c[0])):
        with every_case(failed):
            _filter_case(name, s, prec, rule, launched)
    assert not failed, "\n".join(failed)
    assert launched == want, (sorted(want - launched), sorted(launched - want))


def _filter_case(name, s, prec, rule, launched):
    from mliis_amd import ops
    N, H, W, C, Nout, k = s.N, s.H, s.W, s.K, s.Nout, s.ksize
    sd = seed_of(s._replace(scale=False))       # (the x_scale and plain cases of a plan mostly share a shape: one draw)
    dil = 2 if (k == 3 and sd % 2) else 1
    xg, dyg = gen(N, H, W, C, seed=sd), gen(N, H, W, Nout, seed=sd + 1)
    gg = torch.sigmoid(gen(N, C, seed=sd + 2)) if s.scale else None
    xs = xg * gg[:, None, None, :] if s.scale else xg          # (the product multiplies in fp32, then converts)
    xq, dyq = rounded(xs, rule), rounded(dyg, rule)
    if k == 1:
        w0 = torch.zeros(C, Nout, dtype=torch.float64, requires_grad=True)
        (gw,) = torch.autograd.grad(xq.reshape(-1, C) @ w0, [w0], dyq.reshape(-1, Nout))
        gw = gw.reshape(1, 1, C, Nout)
    else:
        w0 = torch.zeros(3, 3, C, Nout, dtype=torch.float64, requires_grad=True)
        (gw,) = torch.autograd.grad(R.conv2d_same(nchw(xq), w0, 1, dil), [w0], nchw(dyq))
    tmf, nt, mt = CI.filter_plan(s)[:3]
    assert CI.filter_name(tmf, nt, s.scale, prec, mt) == name, (name, s)
    launched.add(name)
    got = ops.conv2d_bwd_filter(xg, dyg, k, dil, x_scale=gg, precision=prec)
    close(got, gw, BWD_TOL, "{} {}".format(name, tuple(s)))
